"""The pyramid kernels' shared row loop (orbfe_extract.hip: col_group / hsum4 / row_entry /
resize4 in resize_kernel, both passes of resize2_kernel, resize_tail_kernel and pyramid_kernel)
at the places it can go wrong.  Every level of every checked frame must be byte-exact against
the oracle's cascaded cv::resize under the matching arithmetic reading.

Frame sizes (level sizes at 1.2 x 8 in brackets, from the oracle):
  50 x 40    [50, 42, 35, 29, 24, 20, 17, 14]: tail levels narrower than 16 bytes;
  97 x 73   [97, 81, 67, 56, 47, 39, 32, 27]: last column groups of 1 and 3 pixels, top levels
             narrower than two 16-byte chunks;
  131 x 99   [131, 109, 91, 76, 63, 53, 44, 37 / 99 .. 33, 28]: last groups of 1 and 3 pixels,
             level 6 is 33 rows (one row in the last 32-row tile);
  258 x 130  [258, 215, 179, 149, 124, 104, 86, 72]: last groups of 2, 3 and 1 pixels;
  643 x 481  [643, 536, 447, 372, 310, 258, 215, 179 / 481 .. 193, 161, 134]: two tile columns,
             levels 5 and 6 leave one row in the last tile, the 640 x 480 tail (levels 5-7);
  345 x 80   [345, 288, 240, 200, 166, 139, 116, 96]: tail levels that are whole column groups
             (the window read of the last group ends at the row's last dword).
In every one the last output row of each level reads the last source row as its second row, and
the last one or two column groups of each level lie past the x86 body bound.  The second source
row clamped onto the first needs two levels of the same height, which only scale factors near 1
reach: 64 x 16 at 1.1 x 10 (levels 8 and 9 are both 7 rows).

Batches of 9 run resize_tail_kernel (>= 8 frames), single frames the level pairs and
resize_kernel for every level."""
import numpy as np
import pytest

import oracle
from orbslam_mapsave_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu

SIZES = [(50, 40), (97, 73), (131, 99), (258, 130), (643, 481), (345, 80)]


def _levels_exact(e, p, imgs, frames, var):
    for f in frames:
        with oracle.variant(var):
            levels = oracle.pyramid(p, imgs[f])
        for l, lev in enumerate(levels):
            g = e.get_level(l, f)
            assert g.shape == lev.shape
            bad = np.argwhere(g != lev)
            assert bad.size == 0, f"frame {f} level {l} {lev.shape}: {len(bad)} px differ, first {bad[:4].tolist()}"


def _run(size, batch, arith, sf=1.2, nl=8, path="per_level", tail=None):
    """Extracts `batch` frames of `size` and checks the levels of the first, a middle and the last
    frame; then one single frame through the same extractor.  `tail`: the expected form of the
    tail kernel for the batch (None: not asserted)."""
    from orbslam_mapsave_amd.native import ORBextractor
    w, h = size
    p = oracle.params(500, sf, nl, 20, 7)
    e = ORBextractor(500, sf, nl, 20, 7, device=0, max_width=w, max_height=h)
    var = oracle.VAR_H5_SSE2 if arith == "x86" else 0
    e.set_arithmetic(e.ARITH_X86_SIMD if arith == "x86" else e.ARITH_SCALAR)
    try:
        imgs = np.stack([synthetic_frame(5 * w + h + s, w, h) for s in range(max(batch, 2))])
        if batch > 1:
            e.extract_batch(imgs)
            assert e.pyramid_path(batch) == path
            if tail is not None:
                assert e.pyramid_tail(batch) == tail
            _levels_exact(e, p, imgs, sorted({0, batch // 2, batch - 1}), var)
        e(imgs[1])
        assert e.pyramid_path(1) == path
        assert e.pyramid_tail(1) == "none"
        _levels_exact(e, p, imgs[1:2], [0], var)
    finally:
        e.close()


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("batch", [1, 9])
@pytest.mark.parametrize("arith", ["scalar", "x86"])
def test_per_level_default(size, batch, arith, monkeypatch):
    """Level pairs (resize2_kernel), the odd level (resize_kernel) and the tail on the
    column-group tables."""
    monkeypatch.setenv("ORBFE_PYR", "0")
    for v in ("ORBFE_RS2", "ORBFE_RESIZE_TABLE"):
        monkeypatch.delenv(v, raising=False)
    _run(size, batch, arith, tail="table")


@pytest.mark.parametrize("size", [(131, 99), (643, 481)])
@pytest.mark.parametrize("arith", ["scalar", "x86"])
@pytest.mark.parametrize("rs2,table", [("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")])
def test_per_level_switches(size, arith, rs2, table, monkeypatch):
    """ORBFE_RS2=0: one resize_kernel launch per level; ORBFE_RESIZE_TABLE=0: resize_kernel and
    the tail by byte gathers (no level pairs)."""
    monkeypatch.setenv("ORBFE_PYR", "0")
    monkeypatch.setenv("ORBFE_RS2", rs2)
    monkeypatch.setenv("ORBFE_RESIZE_TABLE", table)
    _run(size, 9, arith, tail="table" if table == "1" else "gather")


@pytest.mark.parametrize("size", [(97, 73), (258, 130), (643, 481)])
@pytest.mark.parametrize("batch", [1, 9])
@pytest.mark.parametrize("arith", ["scalar", "x86"])
def test_band_kernel(size, batch, arith, monkeypatch):
    """pyramid_kernel (ORBFE_PYR=2: at every size and batch) on the same row loop."""
    monkeypatch.setenv("ORBFE_PYR", "2")
    _run(size, batch, arith, path="bands", tail="none")


@pytest.mark.parametrize("sf,nl", [(1.2, 8), (1.5, 5), (2.0, 4), (1.1, 10)])
@pytest.mark.parametrize("arith", ["scalar", "x86"])
def test_scale_factors_per_level(sf, nl, arith, monkeypatch):
    """Other scale factors on the per-level path: whichever form their plan gives the tail (the
    tables where every group's source columns fit the 8-byte window, else the gathers), the
    levels are exact; at 1.2 the tail runs on the tables."""
    monkeypatch.setenv("ORBFE_PYR", "0")
    for v in ("ORBFE_RS2", "ORBFE_RESIZE_TABLE"):
        monkeypatch.delenv(v, raising=False)
    _run((331, 247), 9, arith, sf=sf, nl=nl, tail="table" if sf == 1.2 else None)


@pytest.mark.parametrize("table", ["1", "0"])
@pytest.mark.parametrize("arith", ["scalar", "x86"])
def test_last_row_clamped(table, arith, monkeypatch):
    """64 x 16 at 1.1 x 10: levels 8 and 9 are both 7 rows, so every row of level 9 has weight 0
    on its second source row and the last one clamps it onto the first."""
    monkeypatch.setenv("ORBFE_PYR", "0")
    monkeypatch.setenv("ORBFE_RESIZE_TABLE", table)
    p = oracle.params(500, 1.1, 10, 20, 7)
    hs = [lev.shape[0] for lev in oracle.pyramid(p, np.zeros((16, 64), np.uint8))]
    assert hs[8] == hs[9]
    _run((64, 16), 9, arith, sf=1.1, nl=10)
