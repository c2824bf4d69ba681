"""Many-tests gradients without a GPU: the header include/fvvdp_hip_tests_grad.h and its binding, the workspace layout and the
argument checks of its entry points, the code objects of tests_ref_layer_kernel, the plane count behind the backward batch and
the refusals of fvvdp.jod_tests that come before any device work."""
import ctypes
import os
import re

import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd import tests_grad as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (vector registers, scalar registers) of tests_ref_layer_kernel<NT> as DESIGN.md section 4, "Gradients of many tests per
# reference", states them
REGS = {1: (35, 34), 2: (39, 42), 4: (47, 44)}
NAMES = ["fvvdp_tests_ref_grad_finish", "fvvdp_tests_ref_grad_layer", "fvvdp_tests_ref_grad_workspace"]


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_header_is_exported_and_bound():
    nat.build()
    assert declared("fvvdp_hip_tests_grad.h") == NAMES
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert sorted(nat.TESTS_GRAD_SYMBOLS) == NAMES
    tables = {k: v for k, v in vars(nat).items() if k.endswith("SYMBOLS") and isinstance(v, dict)}
    assert "TESTS_GRAD_SYMBOLS" in tables and len(tables) >= 15
    for k, v in tables.items():
        if k != "TESTS_GRAD_SYMBOLS":
            assert not set(NAMES) & set(v), k
    # the other headers are as they were: none of them declares the new names
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "fvvdp_hip_tests_grad.h":
            assert not set(NAMES) & set(declared(h)), h
    lib = nat.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    assert nat.TESTS_GRAD_GROUP_MAX == 4
    assert "FVVDP_TESTS_GRAD_GROUP_MAX 4" in open(os.path.join(ROOT, "include", "fvvdp_hip_tests_grad.h")).read()
    # the helpers the new unit shares with the other backward units stay internal
    for name in ("video_coef_launch", "video_level0_launch", "grad_sweep_launch", "ref_grad_layout", "check_slopes"):
        assert not hasattr(L, name), name


def test_workspace_is_the_reference_layout_plus_coefficients():
    lib = nat.lib()
    nbytes, one = ctypes.c_size_t(0), ctypes.c_size_t(0)
    ws = lib.fvvdp_tests_ref_grad_workspace
    assert ws(64, 48, 4, 3, 5, None) == -1 and b"null" in lib.fvvdp_last_error()
    for args in ((64, 48, 0, 3, 5), (64, 48, 17, 3, 5), (64, 48, 4, 0, 5), (0, 48, 4, 3, 5), (64, 0, 4, 3, 5)):
        assert ws(*args, ctypes.byref(nbytes)) == -1 and b"bad shape" in lib.fvvdp_last_error(), args
    for T in (0, -3):
        assert ws(64, 48, 4, 3, T, ctypes.byref(nbytes)) == -1 and b"n_tests" in lib.fvvdp_last_error()
    al = lambda x: (x + 63) // 64 * 64               # noqa: E731
    prev = 0
    for n in (1, 2, 3, 7, 30):                       # monotone in n; the tests add their coefficients and nothing else
        assert lib.fvvdp_ref_grad_workspace(64, 48, 4, n, 2, ctypes.byref(one)) == 0
        for T in (1, 5, 17):
            assert ws(64, 48, 4, n, T, ctypes.byref(nbytes)) == 0
            assert nbytes.value == one.value + 4 * T * al(n * 2 * 4)
        assert nbytes.value > prev
        prev = nbytes.value


def _structs():
    prm, pp = nat.Params(), nat.PoolParams(1, 0.67, 1, 0.25, -0.016, 0.6)
    prm.beta = 0.96
    return prm, pp


def _maps(n_sets, n_bands=4, hole=None):
    maps = (nat.BandMaps * (n_sets * n_bands))()
    for i in range(n_sets * n_bands):
        maps[i].d_D = maps[i].d_contrast = maps[i].d_lbkg = maps[i].d_S = 256
    if hole is not None:
        maps[hole].d_contrast = None
    return maps


def test_layer_argument_checks_need_no_device():
    lib = nat.lib()
    prm, pp = _structs()
    p = ctypes.c_void_p(256)
    slopes = (ctypes.c_void_p * 4)(256, 256, 256, 256)

    def call(n_bands=4, n=2, T=3, test0=0, ng=3, cap=0, add=0, pool=pp, Q=p, n_frames=5, f0=0, gamma=p, mp=None, sl=slopes,
             work_ptr=256, work=1 << 30):
        mp = _maps(max(ng, 1)) if mp is None else mp
        return lib.fvvdp_tests_ref_grad_layer(64, 48, n_bands, n, T, test0, ng, cap, add, ctypes.byref(prm), ctypes.byref(pool), Q,
                                              n_frames, f0, gamma, mp, sl, ctypes.c_void_p(work_ptr), work, None)

    err = lib.fvvdp_last_error
    assert lib.fvvdp_tests_ref_grad_layer(64, 48, 4, 2, 3, 0, 3, 0, 0, None, None, None, 5, 0, None, None, None, None, 0, None) == -1
    assert b"null" in err()
    for kw in ({"Q": None}, {"gamma": None}, {"sl": None}, {"work_ptr": 0}):
        assert call(**kw) == -1 and b"null" in err(), kw
    assert call(n_bands=17) == -1 and b"bad shape" in err()
    assert call(n_bands=0) == -1 and b"bad shape" in err()
    assert call(n=0) == -1 and b"bad shape" in err()
    for T in (0, -2):
        assert call(T=T) == -1 and b"n_tests" in err()
    for kw in ({"test0": -1}, {"ng": 0}, {"ng": 4}, {"test0": 1, "ng": 3}, {"test0": 3, "ng": 1}):
        assert call(**kw) == -1 and b"outside the 3 tests" in err(), kw
    for cap in (3, 5, 8, -1):
        assert call(cap=cap) == -1 and b"group_max" in err(), cap
    assert call(add=2) == -1 and b"add must" in err()
    assert call(f0=4) == -1 and b"outside the clip" in err()
    assert call(f0=-1) == -1 and b"outside the clip" in err()
    assert call(n_frames=1) == -1 and b"outside the clip" in err()
    assert call(pool=nat.PoolParams(1, 0.67, 0, 0.25, -0.016, 0.6)) == -1 and b"exponents" in err()
    assert call(mp=_maps(3, hole=0)) == -1 and b"every map" in err()
    assert call(mp=_maps(3, hole=2 * 4 + 3)) == -1 and b"every map" in err()          # the last band of the third test
    gap = (ctypes.c_void_p * 4)(256, 256, None, 256)
    assert call(sl=gap) == -1 and b"slope plane" in err()
    odd = (ctypes.c_void_p * 4)(256, 258, 256, 256)
    assert call(sl=odd) == -1 and b"slope plane" in err()
    assert call(Q=ctypes.c_void_p(258)) == -1 and b"aligned to 4" in err()
    assert call(work=16) == -1 and b"workspace" in err()
    assert call(work_ptr=260) == -1 and b"aligned" in err()
    # the workspace of T tests is needed, not that of one
    need, one = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.fvvdp_tests_ref_grad_workspace(64, 48, 4, 2, 3, ctypes.byref(need)) == 0
    assert lib.fvvdp_ref_grad_workspace(64, 48, 4, 2, 2, ctypes.byref(one)) == 0
    assert call(work=one.value) == -1 and b"workspace" in err()
    assert call(work=need.value - 1) == -1 and b"workspace" in err()


def test_finish_argument_checks_need_no_device():
    lib = nat.lib()
    err = lib.fvvdp_last_error

    def call(n_bands=4, n=2, T=3, n_frames=5, f0=0, g0=256, work_ptr=256, work=1 << 30):
        return lib.fvvdp_tests_ref_grad_finish(64, 48, n_bands, n, T, n_frames, f0, ctypes.c_void_p(g0), ctypes.c_void_p(work_ptr),
                                               work, None)

    assert call(g0=0) == -1 and b"null" in err()
    assert call(work_ptr=0) == -1 and b"null" in err()
    assert call(n_bands=17) == -1 and b"bad shape" in err()
    assert call(n=0) == -1 and b"bad shape" in err()
    assert call(T=0) == -1 and b"n_tests" in err()
    assert call(f0=4) == -1 and b"outside the clip" in err()
    assert call(f0=-1) == -1 and b"outside the clip" in err()
    assert call(g0=258) == -1 and b"d_g0" in err()
    assert call(work_ptr=260) == -1 and b"aligned" in err()
    need = ctypes.c_size_t(0)
    assert lib.fvvdp_tests_ref_grad_workspace(64, 48, 4, 2, 3, ctypes.byref(need)) == 0
    assert call(work=need.value - 1) == -1 and b"workspace" in err()


def test_layer_kernels_exist_once_do_not_spill_and_match_the_design():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    seen, count = {}, {nt: 0 for nt in REGS}
    for m, n in zip(names, nice):
        k = re.match(r"void tests_ref_layer_kernel<(\d+)>\(", n)
        if not k:
            continue
        nt, x = int(k.group(1)), md[m]
        count[nt] = count.get(nt, 0) + 1
        assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
        assert x.get("agpr_count", 0) == 0 and x["group_segment_fixed_size"] == 0, n
        assert x["vgpr_count"] <= 64, n                         # eight waves per SIMD: the occupancy of a pointwise stream
        seen[nt] = (x["vgpr_count"], x["sgpr_count"])
        print(n.split("(")[0], "VGPRs", x["vgpr_count"], "SGPRs", x["sgpr_count"])
    assert count == {1: 1, 2: 1, 4: 1}
    assert seen == REGS
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("Gradients of many tests per reference"):]
    for nt, (v, sg) in REGS.items():
        assert re.search(r"\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|" % (nt, v, sg), sec), (nt, v, sg)
    # the kernels the new unit includes or launches through the other units are still defined once
    for k in ("void ref_layer_kernel<1>", "void ref_layer_kernel<2>", "video_coef_kernel", "video_layer_kernel",
              "video_level0_kernel", "adj_sweep_kernel", "grad_coef_kernel", "adj_layer_kernel", "grad_input_kernel"):
        assert sum(1 for n in nice if n.split("(")[0] == k) == 1, k


def test_plane_count_behind_the_batch_size():
    assert tg.tests_grad_planes("tests", 1) == tg.tests_grad_planes("tests", 4) == 13      # jod_video's test side
    assert [tg.tests_grad_planes("reference", s) for s in (1, 2, 3, 4)] == [19, 25, 31, 37]
    assert [tg.tests_grad_planes("both", s) for s in (1, 2, 3, 4)] == [23, 29, 35, 41]
    with pytest.raises(ValueError):
        tg.tests_grad_planes("test", 1)
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    assert [tg.map_sets(m, T) for T in (1, 2, 3, 4, 5, 9)] == [1, 2, 3, 4, 4, 4]
    m.tests_grad_sets = 2
    assert [tg.map_sets(m, T) for T in (1, 2, 3, 9)] == [1, 2, 2, 2]
    m.tests_grad_sets = 0
    assert tg.map_sets(m, 5) == 1
    assert tg.GROUP_MAX == 0


def test_jod_tests_refusals_without_device():
    x = [torch.rand((1, 3, 4, 32, 48)) for _ in range(3)]
    r = torch.rand((1, 3, 4, 32, 48))
    kw = dict(frames_per_second=30)
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    for bad in ("test", "refs", None, ""):
        with pytest.raises(ValueError, match='wrt must be "tests", "reference" or "both"'):
            m.jod_tests(x, r, wrt=bad, **kw)
    # what predict_tests refuses
    with pytest.raises(RuntimeError, match="non-foveated"):
        fv.fvvdp(display_name="standard_4k", foveated=True, device="cpu", quiet=True).jod_tests(x, r, **kw)
    with pytest.raises(RuntimeError, match="makes no heat maps"):
        fv.fvvdp(display_name="standard_4k", heatmap="threshold", device="cpu", quiet=True).jod_tests(x, r, **kw)
    from fovvideovdp_amd.video_source import fvvdp_video_source_array
    src = fvvdp_video_source_array(x[0], r, 30, dim_order="BCFHW")
    for tests, ref in (([src], r), (src, r), (x, src)):
        with pytest.raises(RuntimeError, match="takes arrays or tensors"):
            m.jod_tests(tests, ref, **kw)
    for tests in ([], (), x[0], None):
        with pytest.raises(RuntimeError, match="list or tuple of at least one clip"):
            m.jod_tests(tests, r, **kw)
    with pytest.raises(RuntimeError, match="at least 2 frames"):
        m.jod_tests([t[:, :, :1] for t in x], r[:, :, :1], **kw)
    # what jod_video refuses
    with pytest.raises(RuntimeError, match="gradients with respect to the reference are not supported"):
        m.jod_tests(x, r.clone().requires_grad_(True), **kw)
    with pytest.raises(RuntimeError, match='wrt="reference" treats the test as a constant'):
        m.jod_tests([x[0], x[1].clone().requires_grad_(True)], r.clone().requires_grad_(True), wrt="reference", **kw)
    with pytest.raises(RuntimeError, match="float32"):
        m.jod_tests([(t * 255).to(torch.uint8) for t in x], (r * 255).to(torch.uint8), **kw)
    with pytest.raises(RuntimeError, match="float32"):
        m.jod_tests([x[0], x[1].double()], r, **kw)
    with pytest.raises(RuntimeError, match="float32"):
        m.jod_tests(x, r.double(), **kw)
    with pytest.raises(RuntimeError, match="same shape"):
        m.jod_tests([x[0], x[1][..., :40]], r, **kw)
    with pytest.raises(RuntimeError, match="B must be 1"):
        m.jod_tests([torch.rand((2, 3, 4, 32, 48))], torch.rand((2, 3, 4, 32, 48)), **kw)
    with pytest.raises(RuntimeError, match="frames_per_second"):
        m.jod_tests(x, r)
    with pytest.raises(RuntimeError, match="frame rate too high"):
        m.jod_tests(x, r, frames_per_second=300)
    with pytest.raises(RuntimeError, match="colour channels"):
        m.jod_tests([t[:, :2] for t in x], r[:, :2], **kw)
    with pytest.raises(RuntimeError, match="dim_order"):
        m.jod_tests(x, r, dim_order="BCFHH", **kw)

    class Photometry(fv.fvvdp_display_photometry):
        def forward(self, V):
            return V * 100.0

        def get_peak_luminance(self):
            return 100.0

        def get_black_level(self):
            return 0.1

    user = fv.fvvdp(display_name="standard_4k", display_photometry=Photometry(), device="cpu", quiet=True)
    with pytest.raises(RuntimeError, match="closed form"):
        user.jod_tests(x, r, **kw)
    # past the checks every wrt reaches the device, and a CPU metric has none: no CPU fallback
    for wrt, tests, ref in (("tests", [x[0].clone().requires_grad_(True), x[1]], r),
                            ("reference", x, r.clone().requires_grad_(True)),
                            ("both", [x[0].clone().requires_grad_(True)], r.clone().requires_grad_(True)),
                            ("tests", [x[0].half(), x[1]], r.bfloat16()),
                            ("tests", tuple(t[0].permute(1, 2, 3, 0).numpy() for t in x), r[0].permute(1, 2, 3, 0).numpy())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.jod_tests(tests, ref, wrt=wrt, dim_order="BCFHW" if torch.is_tensor(ref) else "FHWC", **kw)


def test_predict_tests_and_jod_tests_share_one_launch_loop():
    import inspect
    from fovvideovdp_amd import multitest
    assert "launch_passes(" in inspect.getsource(multitest._on_device)
    assert "launch_passes(" in inspect.getsource(tg._forward)
    src = inspect.getsource(multitest) + inspect.getsource(tg)
    assert src.count("fvvdp_bands_forward_tests_pool(") == 1 and src.count("lib.fvvdp_bands_forward_tests(") == 1
