"""Many tests per reference without a GPU: the C header fvvdp_hip_tests.h and its binding, the argument checks that need no
context, the workspace layout, the host helper that maps tests to quads, slots and launch groups, the code objects of the new
kernel, and the refusals of fvvdp.predict_tests that come before any device work.  (The checks that need a context are in
tests/test_gpu_multitest.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.multitest import quad_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (vector registers, accumulation registers) of multitest_kernel<NQ, RX, SPLIT> as DESIGN.md section 4, "Many tests per reference",
# states them
REGS = {(1, True, False): (137, 0), (2, False, False): (208, 0), (2, True, False): (229, 0), (3, False, False): (338, 82),
        (3, True, False): (344, 88), (1, True, True): (145, 0), (2, False, True): (219, 0), (2, True, True): (249, 0),
        (3, False, True): (356, 100), (3, True, True): (378, 122)}


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_tests_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_tests.h")
    assert names == ["fvvdp_bands_forward_tests", "fvvdp_bands_forward_tests_pool", "fvvdp_tests_workspace"]
    assert sorted(nat.MULTITEST_SYMBOLS) == names
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    tables = [getattr(nat, t) for t in dir(nat) if t.endswith("SYMBOLS") and t != "MULTITEST_SYMBOLS"]
    assert len(tables) >= 13
    for tab in tables:
        assert not set(names) & set(tab)
    assert len(declared("fvvdp_hip.h")) == 24 == len(nat.SYMBOLS)
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    txt = open(os.path.join(ROOT, "include", "fvvdp_hip_tests.h")).read()
    assert int(re.search(r"#define FVVDP_TESTS_GROUP_MAX (\d+)", txt).group(1)) == nat.TESTS_GROUP_MAX == max(k[0] for k in REGS)


def test_a_null_context_is_refused_without_a_device():
    lib = nat.lib()
    pp = nat.PoolParams(1, 0.67, 1, 0.25, -0.016, 0.6)
    assert lib.fvvdp_bands_forward_tests(None, 2, 3, None, 2, 0, None, 0, None) == -1
    assert b"null" in lib.fvvdp_last_error()
    assert lib.fvvdp_bands_forward_tests_pool(None, 2, 3, None, 2, 0, None, 0, ctypes.byref(pp), None, None) == -1
    assert b"null" in lib.fvvdp_last_error()
    assert lib.fvvdp_bands_forward_tests_pool(None, 2, 3, None, 2, 0, None, 0, None, None, None) == -1
    assert b"null" in lib.fvvdp_last_error()


def test_workspace_matches_its_documented_layout():
    lib = nat.lib()
    nbytes = ctypes.c_size_t(0)
    assert lib.fvvdp_tests_workspace(64, 48, 4, 5, 3, None) == -1 and b"null" in lib.fvvdp_last_error()
    for bad in ((0, 48, 4, 5, 3), (64, 0, 4, 5, 3), (64, 48, 0, 5, 3), (64, 48, 17, 5, 3), (64, 48, 4, 0, 3), (64, 48, 4, 5, 0),
                (64, 48, 4, -1, 3)):
        assert lib.fvvdp_tests_workspace(*bad, ctypes.byref(nbytes)) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert lib.fvvdp_tests_workspace(64, 48, 4, 5, 3, ctypes.byref(nbytes)) == 0
    # one strip per level.  One-level walk of bands 0..3: ceil(hc / 2) chunks at the most = 12, 6, 3, 2; a two-level walk of
    # bands (b, b + 1) has one chunk per row of level b + 2 at the most = 12, 6, 3 for b = 0, 1, 2; a band takes the largest
    one, two = [12, 6, 3, 2], [12, 6, 3]
    blk = [max([one[b]] + [two[a] for a in (b - 1, b) if 0 <= a < 3]) for b in range(4)]
    assert blk == [12, 12, 6, 3]
    row = (sum(3 * b * 2 for b in blk) + 63) // 64 * 64
    assert nbytes.value == 5 * row * 4
    assert lib.fvvdp_tests_workspace(3840, 2160, 1, 2, 1, ctypes.byref(nbytes)) == 0
    assert nbytes.value == 2 * ((32 * 540 * 2 + 63) // 64 * 64) * 4
    # two bands of a 4K frame: 32 / 16 one-level strips x ceil(hc / 2) chunks against ceil(1920 / 54) = 36 two-level strips x 540
    # level-C rows -- the larger bound of either band
    assert lib.fvvdp_tests_workspace(3840, 2160, 2, 3, 2, ctypes.byref(nbytes)) == 0
    blk = [max(32 * 540, 36 * 540), max(16 * 270, 36 * 540)]
    assert nbytes.value == 3 * ((sum(2 * b * 2 for b in blk) + 63) // 64 * 64) * 4


@pytest.mark.parametrize("group_max", [2, 3])
@pytest.mark.parametrize("T", list(range(1, 10)))
def test_quads_slots_and_groups(T, group_max):
    n = 5
    qp = quad_plan(T, n, group_max)
    assert qp.n_quads == -(-(T + 1) // 2) and len(qp.quads) == qp.n_quads
    assert qp.slot0 == [q * n for q in range(qp.n_quads)]           # quad q: frame slots [q n, q n + n)
    # every stream (tests 0 .. T-1, the reference T) is in exactly one quad component -- except that an even T repeats the
    # reference in the last quad; the reference is component (y, w) of the last quad in every case
    comps = [s for quad in qp.quads for s in quad]
    for s in range(T):
        assert comps.count(s) == 1
    assert comps.count(T) == (1 if T % 2 else 2)
    assert qp.quads[-1][1] == T and qp.ref_quad == qp.n_quads - 1
    assert all(quad == (2 * q, min(2 * q + 1, T)) for q, quad in enumerate(qp.quads))
    for g in qp.groups:
        assert g['quads'][0] == qp.ref_quad                         # the reference's quad is in every group, first
        assert 1 <= len(g['quads']) <= group_max and len(set(g['quads'])) == len(g['quads'])
        assert set(g['store']) <= set(g['quads'])
        # a group evaluates exactly the tests of its other quads, the first one also the test beside the reference
        want = sorted(s for q in g['quads'][1:] for s in qp.quads[q])
        if g is qp.groups[0] and T % 2:
            want = sorted(want + [T - 1])
        assert sorted(g['tests']) == want
    stores = [q for g in qp.groups for q in g['store']]
    assert sorted(stores) == list(range(qp.n_quads))                # every quad's next level is written by exactly one group
    tests = [t for g in qp.groups for t in g['tests']]
    assert sorted(tests) == list(range(T))                          # every test is evaluated by exactly one group
    assert len(qp.groups) == max(1, -(-(qp.n_quads - 1) // (group_max - 1)))


def test_quad_plan_refuses_nonsense():
    for bad in ((0, 3), (3, 0), (-1, 2)):
        with pytest.raises(ValueError):
            quad_plan(*bad)


def test_new_kernels_do_not_spill_and_hold_the_stated_registers():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    counted = ("band_kernel<", "band2_kernel<", "band2_fov_kernel<", "temporal_vec_kernel<", "temporal_ring_kernel<", "temporal_yuv",
               "still_ingest_kernel<", "pu21_sse_kernel<", "multigaze_kernel<")          # substrings other tests count kernels by
    seen = {}
    for m, n in zip(names, nice):
        if "multitest_kernel<" not in n:
            continue
        x = md[m]
        assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
        assert not any(h in n for h in counted), n
        k = re.search(r"multitest_kernel<(\d+), (true|false), (true|false)>", n)
        seen[(int(k.group(1)), k.group(2) == "true", k.group(3) == "true")] = (x["vgpr_count"], x.get("agpr_count", 0))
        assert x["vgpr_count"] + x.get("agpr_count", 0) <= 512          # one wave per SIMD at the least
        if int(k.group(1)) <= 2:
            assert x["vgpr_count"] <= 256 and x.get("agpr_count", 0) == 0      # two waves per SIMD
    assert seen == REGS                                              # ten instantiations
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("Many tests per reference"):]
    for (nq, rx, split), (v, acc) in REGS.items():
        assert re.search(r"\|\s*%d\s*\|\s*%s\s*\|\s*%s\s*\|\s*%d\s*\|\s*%d\s*\|" % (
            nq, "yes" if rx else "no", "yes" if split else "no", v, acc), sec), (nq, rx, split, v, acc)


def test_refusals_before_any_device_work():
    a = np.zeros((1, 1, 3, 64, 64), np.float32)
    cpu = fv.fvvdp(display_name="standard_4k", device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu.predict_tests([a, a], a, frames_per_second=30)
    with pytest.raises(RuntimeError, match="foveated.*predict\\(\\)"):
        fv.fvvdp(display_name="standard_4k", foveated=True, device=torch.device("cpu")).predict_tests([a], a, frames_per_second=30)
    with pytest.raises(RuntimeError, match="fixation_point.*predict\\(\\)"):
        cpu.predict_tests([a], a, frames_per_second=30, fixation_point=[10, 10])
    with pytest.raises(RuntimeError, match="heat maps"):
        fv.fvvdp(display_name="standard_4k", heatmap="raw", device=torch.device("cpu")).predict_tests([a], a, frames_per_second=30)
    one = np.zeros((1, 1, 1, 64, 64), np.float32)
    with pytest.raises(RuntimeError, match="predict_images"):
        cpu.predict_tests([one], one, frames_per_second=30)
    with pytest.raises(RuntimeError, match="shape or dtype.*predict\\(\\)"):
        cpu.predict_tests([a, np.zeros((1, 1, 3, 64, 66), np.float32)], a, frames_per_second=30)
    with pytest.raises(RuntimeError, match="shape or dtype.*predict\\(\\)"):
        cpu.predict_tests([a.astype(np.float16)], a, frames_per_second=30)
    with pytest.raises(RuntimeError, match="shape or dtype"):
        cpu.predict_tests([torch.zeros((1, 1, 3, 64, 64), dtype=torch.uint8)], a, frames_per_second=30)
    for bad in ([], (), a, None):
        with pytest.raises(RuntimeError, match="list or tuple"):
            cpu.predict_tests(bad, a, frames_per_second=30)
    x = torch.zeros((1, 1, 3, 64, 64), requires_grad=True)
    with pytest.raises(RuntimeError, match="Gradients"):
        cpu.predict_tests([x.detach(), x], x.detach(), frames_per_second=30)
    with pytest.raises(RuntimeError, match="Gradients"):
        cpu.predict_tests([x.detach()], x, frames_per_second=30)
    vs = fv.fvvdp_video_source_array(a, a, 30, display_photometry=cpu.display_photometry)
    with pytest.raises(RuntimeError, match="predict_video_source"):
        cpu.predict_tests([vs], a, frames_per_second=30)
    with pytest.raises(RuntimeError, match="predict_video_source"):
        cpu.predict_tests(vs, a, frames_per_second=30)
    with pytest.raises(RuntimeError, match="predict_video_source"):
        cpu.predict_tests([a], vs, frames_per_second=30)
    # uint16 carried by numpy and a torch int16 tensor of the same bits are one sample type: past the checks, to the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu.predict_tests((np.zeros((1, 3, 2, 64, 64), np.uint16),), torch.zeros((1, 3, 2, 64, 64), dtype=torch.int16), frames_per_second=30)
