"""The arithmetic under the device map's store (csrc/orbfe_map_plan.hpp): tests/cpp/map_store_plan_test.cpp
built alone with AddressSanitizer and UBSan and run as a child process.  Needs no GPU and no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_planner_and_column_growth_under_sanitizers(tmp_path):
    exe = str(tmp_path / "map_store_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "map_store_plan_test.cpp")], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "map_store_plan_test ok" in r.stdout, r.stdout
