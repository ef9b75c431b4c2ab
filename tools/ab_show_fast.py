"""Print the bench lines of $BENCH_OUT/<tag>/ (tools/ab_quick.sh; default bench_out/)."""
import glob, json, os, sys
d = os.path.join(os.environ.get("BENCH_OUT", "bench_out"), sys.argv[1] if len(sys.argv) > 1 else "fstrip")
for f in sorted(glob.glob(os.path.join(d, "c*_s*.json"))):
    j = json.load(open(f))
    s = j["stage_ms_per_step"]
    print(os.path.basename(f), round(j["value"]), j["ms_per_step"], "fast", s["fast"], "resize", s["resize"],
          "describe", s["describe"], "octree", s["octree"])
t = os.path.join(d, "fast_timing.json")
if os.path.exists(t):
    print(open(t).read())
