"""The RGB-D restatement (rgbd_cases.py) checked on the CPU: its built cases reach every branch,
every single-decision mutant changes an answer on them, the closed form of the visited prefix
equals the literal walk, the depth conversion has one reading, and the C entry points refuse bad
arguments without a device."""
import ctypes as C

import numpy as np
import pytest

import rgbd_cases as R
from orbslam_mapsave_amd import abi, native

F32 = np.float32


@pytest.fixture(scope="module")
def stereo_cases():
    return R.stereo_cases()


@pytest.fixture(scope="module")
def close_cases():
    return R.close_cases()


def _close_runs(cases):
    for name, c in cases.items():
        for mode in (R.CLOSE_SORTED, R.CLOSE_ALL):
            yield name, mode, c


@pytest.mark.parametrize("mutant", R.STEREO_MUTANTS)
def test_stereo_mutants_change_an_answer(stereo_cases, mutant):
    changed = [name for name, c in stereo_cases.items()
               if not R.same_bits(R.restated_stereo(*c), R.restated_stereo(*c, mutant=mutant))]
    assert changed, f"no built case tells {mutant} from the reference"


@pytest.mark.parametrize("mutant", R.CLOSE_MUTANTS)
def test_close_mutants_change_an_answer(close_cases, mutant):
    changed = [(name, mode) for name, mode, c in _close_runs(close_cases)
               if not R.same_bits(R.run_close(c, mode), R.run_close(c, mode, mutant=mutant))]
    assert changed, f"no built case tells {mutant} from the reference"


def test_branch_counters(stereo_cases, close_cases):
    st = {}
    for c in stereo_cases.values():
        R.restated_stereo(*c, stats=st)
    for k in ("oob", "frac", "neg_frac", "nan_depth", "d_pos", "d_nonpos", "denormal", "un_distinct"):
        assert st.get(k, 0) >= 5, (k, st)
    st = {}
    for _, mode, c in _close_runs(close_cases):
        R.run_close(c, mode, stats=st)
    for k in ("near", "near_map", "dropped", "created", "has_point", "tie", "beyond_visited",
              "break_fired", "ran_out", "octave_oob"):
        assert st.get(k, 0) >= 5, (k, st)


def test_closed_prefix_is_the_literal_walk(close_cases):
    for name, c in close_cases.items():
        got = R.run_close(c, R.CLOSE_SORTED, dists=False)["n_visited"]
        assert got == R.closed_prefix(c["depth"], c["th"], c["min_points"]), name
    r = np.random.default_rng(3)
    for t in range(300):
        n = int(r.integers(0, 40))
        d = r.choice(np.asarray([0, -1, np.nan, 0.5, 1, 1, 2, 2, 2.5, 3, np.inf], F32), n)
        case = R._close_case(d, r.random(n) < 0.5, t, th=r.choice(np.asarray([0.25, 1, 2, 2.75, np.inf, np.nan], F32)),
                             min_points=int(r.integers(0, 12)))
        got = R.run_close(case, R.CLOSE_SORTED, dists=False)["n_visited"]
        assert got == R.closed_prefix(d, case["th"], case["min_points"]), (t, d, case["th"])


def test_conversion_has_one_reading():
    """convertTo(CV_32F, alpha) = src * alpha + 0: a float multiply, a double multiply rounded
    once and an fma with 0 give the same float for every U16 value (the product of a 16-bit
    integer and a float is exact in double), and for float sources (24 x 24 bits)."""
    raw = np.arange(65536, dtype=np.uint16)
    for f in R.FACTORS:
        got = R.conversion_readings(raw, f)
        assert got["float_mul"].tobytes() == got["double_mul"].tobytes() == got["fma0"].tobytes(), f
    assert R.FACTOR_1000 == F32(0.001) and R.FACTOR_5000 == F32(0.0002)
    r = np.random.default_rng(5)
    src = r.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(F32)
    src = src[np.isfinite(src)]
    for f in R.FACTORS:
        got = R.conversion_readings(src, f)
        a, b = got["float_mul"], got["double_mul"]
        keep = ~np.isnan(a)
        # +0 only turns -0 into +0, and d > 0 never stores either
        assert np.array_equal(a[keep], b[keep]) and np.array_equal(a[keep], got["fma0"][keep]), f
        assert np.array_equal(np.isnan(a), np.isnan(b))


def test_bad_arguments_are_refused_without_a_device():
    L = native.lib()
    k = R.keys_at([1.0], [1.0])
    img = np.zeros((4, 4), np.uint16)
    out = np.zeros(4, F32)
    p = abi.ptr
    assert L.orbfe_compute_stereo_from_rgbd(None, p(img), 0, 4, 4, 8, 1.0, p(k), None, 1, 40.0,
                                            p(out), p(out)) == abi.ORBFE_ERR_ARG
    assert L.orbfe_compute_stereo_from_rgbd_device(None, 1, p(img), 0, 4, 4, 8, 32, 1.0, p(k), None,
                                                   p(out), 1, 40.0, p(out), p(out)) == abi.ORBFE_ERR_ARG
    buf, stride = C.c_void_p(), C.c_size_t()
    assert L.orbfe_depth_buffer(None, 4, 4, 0, C.byref(buf), C.byref(stride)) == abi.ORBFE_ERR_ARG
    assert L.orbfe_rgbd_status(None) == abi.ORBFE_ERR_ARG
    cam = abi.Camera(500, 500, 320, 240, 40, 0.08)
    i32 = np.zeros(4, np.int32)
    u8 = np.zeros(4, np.uint8)
    args = (p(k), p(out), p(u8), 1, C.addressof(cam), p(R.IDENTITY), 3.0, 100, p(R.SCALE), 8, p(i32),
            p(i32), p(u8), p(out), None, None, p(i32), p(i32))
    assert L.orbfe_close_points(None, R.CLOSE_SORTED, *args) == abi.ORBFE_ERR_ARG
    assert L.orbfe_close_points(None, 7, *args) == abi.ORBFE_ERR_ARG
    assert L.orbfe_close_points_batch_device(None, 0, 1, p(k), p(out), p(u8), p(i32), 1, C.addressof(cam),
                                             p(R.IDENTITY), 3.0, 100, p(R.SCALE), 8, p(i32), p(i32), p(u8),
                                             p(out), None, None, p(i32), p(i32), p(i32)) == abi.ORBFE_ERR_ARG
    assert native.DEPTH_U16 == 0 and native.DEPTH_F32 == 1 and native.CLOSE_MAX_KEPT == 8192
    with pytest.raises(ValueError):
        native._depth_type(np.uint8)
