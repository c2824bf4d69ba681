"""The code objects of the four fused pyramid kernels, without a GPU.  The kernels share their row walk (csrc/pyramid_walk.hpp);
how a shared piece takes its arguments decides the callers' code -- weights passed in a struct by reference once cost
band_kernel scratch memory and LDS traffic -- so every one of the 34 instantiations must stay free of scratch and of vector
spills and inside the registers it had while each kernel carried its own copy of the walk.

The recorded values are those of the build before the walk was shared.  Two map-writing foveated instantiations spilled scalar
registers into vector lanes (no scratch) in that build already: their counts are recorded as bounds as well, every other
instantiation has none."""
import re

from fovvideovdp_amd import _native as nat

# kernel -> {template arguments: (VGPRs, scalar registers spilled into vector lanes)}
RECORDED = {
    "band_kernel": {          # <P, DBG, FOVM>
        (2, False, 0): (78, 0), (2, False, 1): (104, 0), (2, False, 2): (142, 0), (2, False, 3): (136, 0),
        (2, True, 0): (80, 0), (2, True, 2): (114, 12),
        (4, False, 0): (126, 0), (4, False, 1): (165, 0), (4, False, 2): (219, 0), (4, False, 3): (200, 0),
        (4, True, 0): (133, 0), (4, True, 2): (179, 24),
    },
    "band2_kernel": {         # <P, INRANGE>
        (2, False): (100, 0), (2, True): (94, 0), (4, False): (162, 0), (4, True): (158, 0),
    },
    "multigaze_kernel": {     # <P, NG>
        (2, 1): (111, 0), (2, 2): (125, 0), (2, 4): (141, 0), (2, 8): (172, 0),
        (4, 1): (154, 0), (4, 2): (168, 0), (4, 4): (190, 0), (4, 8): (234, 0),
    },
    "multitest_kernel": {     # <NQ, RX, SPLIT>
        (1, True, False): (137, 0), (1, True, True): (145, 0),
        (2, False, False): (208, 0), (2, False, True): (219, 0), (2, True, False): (229, 0), (2, True, True): (249, 0),
        (3, False, False): (338, 0), (3, False, True): (356, 0), (3, True, False): (344, 0), (3, True, True): (378, 0),
    },
}


def _template_args(text):
    return tuple(t.strip() == "true" if t.strip() in ("true", "false") else int(t) for t in text.split(","))


def test_the_34_instantiations_keep_their_registers_and_use_no_scratch():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    seen = {k: {} for k in RECORDED}
    for m, n in zip(names, codeobj.demangle(names)):
        k = re.match(r"(?:void )?(band_kernel|band2_kernel|multigaze_kernel|multitest_kernel)<([^<>]*)>", n)
        if k:
            seen[k.group(1)][_template_args(k.group(2))] = md[m]
    assert sum(len(v) for v in RECORDED.values()) == 34
    for kernel, table in RECORDED.items():
        assert sorted(seen[kernel]) == sorted(table), kernel
        for args, (vgprs, sgpr_spills) in table.items():
            x = seen[kernel][args]
            print(kernel, args, "vgpr", x["vgpr_count"], "<=", vgprs, " sgpr spills", x["sgpr_spill_count"], "<=", sgpr_spills,
                  " scratch", x["private_segment_fixed_size"], " vgpr spills", x["vgpr_spill_count"])
            assert x["private_segment_fixed_size"] == 0, (kernel, args)
            assert x["vgpr_spill_count"] == 0, (kernel, args)
            assert x["sgpr_spill_count"] <= sgpr_spills, (kernel, args)
            assert x["vgpr_count"] <= vgprs, (kernel, args)
