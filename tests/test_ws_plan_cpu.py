"""CPU (-m "not gpu"): the workspace plans of the Winograd convolutions (csrc/winograd.hip) and the x3 transposed convolutions
(csrc/gemm_x3.hip).  The size queries and pdf_debug_workspace_plan are host code, so the layout every launcher carves its buffers
from is checked here without a device:
  * every public size / offset query returns what the library returned before the plans existed (tests/golden/ws_plan_table.json,
    recorded from that library over the grid below under pdf_set_x3_mode 0, 1, 2 and 7);
  * every region of every plan is 16-byte aligned, inside [0, total) and disjoint from the others; a plan that is not ok has total 0;
  * the parity-class tap enumerator (gemm_common.h) yields the taps, order and offsets of the three loops it replaced (a stand-alone
    host program under tests/c_abi, built with the address and undefined-behaviour sanitizers)."""
import ctypes
import json
import os
import subprocess

import pytest

from tests.util import ROOT

MODES = (0, 1, 2, 7)
# (N, H, W, Cin, Cout, KH, KW, stride, pad) of stride-1 3x3 convolutions and their ineligible neighbours
WINO_GRID = [
    # the shapes tests/test_ws_plan_gpu.py runs (fp32 planes; x3 planes; fp32 forward with x3 backward-data; Cout % 32 != 0; F(2x2))
    (2, 64, 64, 128, 64, 3, 3, 1, 1), (2, 128, 128, 256, 256, 3, 3, 1, 1), (2, 128, 128, 128, 256, 3, 3, 1, 1), (2, 128, 128, 256, 80, 3, 3, 1, 1),
    (4, 34, 34, 128, 64, 3, 3, 1, 1),
    # the step's layers at B = 32 (tests/test_headline_gpu.py): feat, the heads and their shared input, the decoders, ResNet layers 2-3
    (32, 64, 64, 1024, 256, 3, 3, 1, 1), (32, 64, 64, 256, 256, 3, 3, 1, 1), (32, 64, 64, 256, 512, 3, 3, 1, 1), (32, 128, 128, 128, 128, 3, 3, 1, 1),
    (32, 32, 32, 128, 128, 3, 3, 1, 1), (32, 16, 16, 256, 256, 3, 3, 1, 1), (32, 32, 32, 256, 256, 3, 3, 1, 1), (8, 16, 16, 256, 256, 3, 3, 1, 1),
    # channel thresholds: Cin below PDF_WINOGRAD_MINC, Cout below 64, counts that are no multiple of 16 / of 32
    (2, 64, 64, 112, 64, 3, 3, 1, 1), (2, 64, 64, 128, 48, 3, 3, 1, 1), (2, 64, 64, 136, 64, 3, 3, 1, 1), (2, 128, 128, 288, 256, 3, 3, 1, 1),
    (2, 128, 128, 256, 272, 3, 3, 1, 1),
    # map edges: H % 4 != 0 (F(2x2)), odd, T % 16 != 0, T % 32 != 0
    (2, 66, 66, 128, 64, 3, 3, 1, 1), (2, 63, 64, 128, 64, 3, 3, 1, 1), (3, 52, 52, 128, 128, 3, 3, 1, 1), (1, 36, 36, 128, 128, 3, 3, 1, 1),
    (2, 120, 120, 256, 256, 3, 3, 1, 1),
    # planes x tiles around PDF_WINOGRAD_MINPT, tiles around PDF_X3_MINT
    (1, 64, 64, 128, 128, 3, 3, 1, 1), (1, 32, 32, 256, 256, 3, 3, 1, 1), (1, 128, 128, 256, 256, 3, 3, 1, 1), (2, 64, 64, 1024, 256, 3, 3, 1, 1),
    (8, 64, 64, 1024, 256, 3, 3, 1, 1),
    # the 32-bit byte offsets of x3 planes, the 4 GB bound of a transform-domain plane
    (32, 128, 128, 1024, 256, 3, 3, 1, 1), (32, 512, 512, 2048, 128, 3, 3, 1, 1),
    # not a stride-1 3x3 convolution
    (2, 64, 64, 128, 64, 1, 1, 1, 0), (2, 64, 64, 128, 64, 3, 3, 2, 1), (2, 64, 64, 128, 64, 3, 3, 1, 0), (2, 64, 64, 128, 64, 3, 1, 1, 1),
]
# (N, H, W, Cin, Cout, KH, KW, stride, pad) of transposed convolutions
X3D_GRID = [
    # the shapes tests/test_ws_plan_gpu.py runs, the smallest over the flop bar of each form
    (1, 64, 64, 1024, 256, 4, 4, 4, 0), (1, 32, 32, 2048, 256, 8, 8, 8, 0), (2, 64, 64, 512, 256, 4, 4, 2, 1),
    # the step's p3 / p4 / p5 at B = 32
    (32, 32, 32, 512, 256, 4, 4, 2, 1), (32, 16, 16, 1024, 256, 4, 4, 4, 0), (32, 8, 8, 2048, 256, 8, 8, 8, 0),
    # M one step below the flop bar / the 1,024-row bar of each form, and the first M above it that the weight gradient refuses
    (1, 59, 60, 1024, 256, 4, 4, 4, 0), (1, 60, 60, 1024, 256, 4, 4, 4, 0), (1, 31, 32, 2048, 256, 8, 8, 8, 0), (1, 64, 64, 512, 256, 4, 4, 2, 1),
    (2, 59, 60, 512, 256, 4, 4, 2, 1), (2, 60, 60, 512, 256, 4, 4, 2, 1), (7, 32, 32, 512, 256, 4, 4, 2, 1),
    # channel counts: no multiple of 32; Cout no multiple of 128 (general weight gradient)
    (1, 64, 64, 1040, 256, 4, 4, 4, 0), (2, 64, 64, 512, 224, 4, 4, 2, 1), (2, 64, 64, 512, 240, 4, 4, 2, 1),
    # kernel / stride / pad: k == s == 2, k no multiple of s, k^2 > 16, stride 1, other pads, KH != KW
    (8, 64, 64, 512, 256, 2, 2, 2, 0), (2, 64, 64, 512, 256, 3, 3, 2, 1), (2, 64, 64, 512, 256, 6, 6, 2, 2), (2, 64, 64, 512, 256, 8, 8, 4, 2),
    (2, 64, 64, 512, 256, 3, 3, 1, 1), (2, 64, 64, 512, 256, 4, 4, 2, 0), (2, 64, 64, 512, 256, 4, 4, 2, 3), (2, 64, 64, 512, 256, 4, 4, 2, 4),
    (1, 64, 64, 1024, 256, 4, 4, 4, 1), (1, 64, 64, 1024, 256, 4, 2, 4, 0),
]
TABLE = os.path.join(ROOT, "tests", "golden", "ws_plan_table.json")


def _key(mode, shape):
    return "%d:%s" % (mode, ",".join(str(v) for v in shape))


def _cdll():
    from pdfnet_amd import hip
    L = ctypes.CDLL(hip.LIB_PATH)
    for name, ret in (("pdf_conv2d_winograd_workspace_floats", ctypes.c_long), ("pdf_conv2d_winograd_v_offset", ctypes.c_long),
                      ("pdf_deconv2d_x3_workspace_floats", ctypes.c_long)):
        getattr(L, name).restype = ret
    return L


def query(L, mode):
    """{key: numbers} of the public size queries over both grids under x3 mode `mode` (also what recorded the table)."""
    L.pdf_set_x3_mode(mode)
    out = {}
    for sh in WINO_GRID:
        out["w" + _key(mode, sh)] = [L.pdf_conv2d_winograd_workspace_floats(*sh, b) for b in (0, 1, 2)] + [L.pdf_conv2d_winograd_v_offset(*sh)]
    for sh in X3D_GRID:
        out["d" + _key(mode, sh)] = [L.pdf_deconv2d_x3_workspace_floats(*sh, b) for b in (0, 1, 2)]
    L.pdf_set_x3_mode(-1)
    return out


def plan(L, kind, pas, shape):
    """pdf_debug_workspace_plan as a dict (include/pdfnet_hip.h lists the fields)."""
    buf = (ctypes.c_long * 32)()
    n = L.pdf_debug_workspace_plan(kind, pas, *shape, buf, 32)
    assert 8 <= n <= 32 and (n - 8) % 2 == 0, n
    names = ("ok", "total", "form", "x3", "splits", "v_offset", "shared_v_x3", "regions")
    d = dict(zip(names, buf[:8]))
    assert d["regions"] == (n - 8) // 2
    d["regions"] = [(buf[8 + 2 * i], buf[9 + 2 * i]) for i in range(d["regions"])]
    return d


def test_size_queries_return_what_they_returned_before_the_plans():
    L = _cdll()
    want = json.load(open(TABLE))
    assert len(want) == len(MODES) * (len(WINO_GRID) + len(X3D_GRID))
    got = {}
    for mode in MODES:
        got.update(query(L, mode))
    bad = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
    assert not bad, bad
    # the anchors, written out: (forward, backward-data, weight gradient, V offset) and (forward, backward-data, weight gradient) at mode 7
    assert want["w7:2,64,64,128,64,3,3,1,1"] == [3833856, 0, 4145280, 294912]
    assert want["w7:2,128,128,256,256,3,3,1,1"] == [50724864, 50724864, 75628864, 3538944]
    assert want["w7:2,128,128,128,256,3,3,1,1"] == [29491200, 39518208, 37880128, 1179648]
    assert want["w7:2,128,128,256,80,3,3,1,1"] == [35315712, 0, 30711952, 1105920]
    assert want["w7:4,34,34,128,64,3,3,1,1"] == [3682304, 0, 0, -1]
    assert want["d7:1,64,64,1024,256,4,4,4,0"] == [13369408, 31948864, 32243776]
    assert want["d7:1,32,32,2048,256,8,8,8,0"] == [55148608, 75792448, 28508224]
    assert want["d7:2,64,64,512,256,4,4,2,1"] == [10322848, 18924064, 31195680]


@pytest.mark.parametrize("mode", MODES)
def test_plan_regions_are_aligned_disjoint_and_inside_the_total(mode):
    L = _cdll()
    L.pdf_set_x3_mode(mode)
    try:
        seen = 0
        for kind, grid, fn in ((0, WINO_GRID, L.pdf_conv2d_winograd_workspace_floats), (1, X3D_GRID, L.pdf_deconv2d_x3_workspace_floats)):
            for sh in grid:
                for pas in (0, 1, 2):
                    p = plan(L, kind, pas, sh)
                    assert p["total"] == fn(*sh, pas), (kind, pas, sh)
                    if not p["ok"]:
                        assert p["total"] == 0 and p["regions"] == [] and p["v_offset"] == -1, (kind, pas, sh, p)
                        continue
                    seen += 1
                    regs = sorted(p["regions"])
                    assert regs and all(ln > 0 for _, ln in regs), (kind, pas, sh, p)
                    for off, ln in regs:
                        assert off % 4 == 0 and 0 <= off and off + ln <= p["total"], (kind, pas, sh, p)
                    for (o0, l0), (o1, _) in zip(regs, regs[1:]):
                        assert o0 + l0 <= o1, (kind, pas, sh, p)
                    if kind == 0 and pas == 0:
                        voff = L.pdf_conv2d_winograd_v_offset(*sh)
                        assert p["v_offset"] == voff, (sh, p)
                        if voff >= 0:                         # the region the weight gradient reads is the forward's V
                            assert p["regions"][1][0] == voff and p["form"] == 4, (sh, p)
                    else:
                        assert p["v_offset"] == -1
                    if kind == 0:                             # a handed-in V is used only in the format the plan records for its own
                        assert p["shared_v_x3"] in (-1, 0, 1) and p["x3"] in (0, 1) and (mode & 1 or p["x3"] == 0), (sh, p)
        assert seen >= (30 if mode & 2 else 20)
    finally:
        L.pdf_set_x3_mode(-1)


def test_weight_gradient_refuses_a_forward_v_in_the_other_format():
    """(2, 128, 128, 256 -> 80): the forward's V is x3 planes (T = 2,048 tiles of 256 channels), the weight gradient's products are fp32
    because Cout % 32 != 0 -- the plan records both formats and they differ; with 256 output channels they agree."""
    L = _cdll()
    L.pdf_set_x3_mode(7)
    try:
        fwd, wg = plan(L, 0, 0, (2, 128, 128, 256, 80, 3, 3, 1, 1)), plan(L, 0, 2, (2, 128, 128, 256, 80, 3, 3, 1, 1))
        assert fwd["x3"] == 1 and wg["x3"] == 0 and wg["shared_v_x3"] == 1 and fwd["v_offset"] == 54 * 256 * 80
        fwd, wg = plan(L, 0, 0, (2, 128, 128, 256, 256, 3, 3, 1, 1)), plan(L, 0, 2, (2, 128, 128, 256, 256, 3, 3, 1, 1))
        assert fwd["x3"] == 1 and wg["x3"] == 1 and wg["shared_v_x3"] == 1
        assert plan(L, 0, 2, (4, 34, 34, 128, 64, 3, 3, 1, 1))["ok"] == 0           # (no F(2x2) weight gradient)
        assert plan(L, 0, 0, (4, 34, 34, 128, 64, 3, 3, 1, 1))["shared_v_x3"] == -1   # an F(2x2) forward takes no shared V
    finally:
        L.pdf_set_x3_mode(-1)


def test_parity_tap_enumerator_matches_the_three_loops_it_replaced(tmp_path):
    """tests/c_abi/parity_taps_check.cpp keeps the three old loops and compares them with pdf_parity_taps over k in {1, 2, 3, 4, 7, 8},
    stride in {1, 2, 4, 8}, pad in 0 .. k - 1, every parity class: same taps, same order, same offsets."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")           # host side only: gemm_common.h includes the HIP headers
    exe = str(tmp_path / "parity_taps_check")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "pdfnet_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_abi", "parity_taps_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "parity taps ok" in r.stdout, r.stdout
