"""Test helper (CPU only): the yardstick, the inputs and the plan restatement of the foveated one-level pixel tests
(tests/test_fov_pixels_cpu.py, tests/test_gpu_fov_pixels.py).  No formula of its own:

- the reference is `orc.Oracle(display, geometry=..., foveated=True, dtype=np.float64)` with `capture`, called per frame through
  `process_frame` on planar [P,H,W] input, and `orc.gausspyr_reduce(..., np.float64)` for the Gaussian levels;
- `band_strips` / `chunking` restate the host's work decomposition (pyramid_host.hpp) so that a test can say, without a GPU, which
  loop phases of band_item a shape reaches, and `parse_plans` reads the FVVDP_DEBUG_VARIANT line of every one-level launch."""
import functools
import re

import numpy as np

from oracle import fvvdp_oracle as orc

F64 = np.float64
N_FRAMES = 5
STRIP_J = 60                      # coarse columns a strip advances by (pyramid_constants.hpp)
WAVE_CAPACITY = 4096              # 16 resident single-wave workgroups x 256 CUs (MI355X); fewer on any smaller part

# (H, W): the smallest shapes with an interior strip at level 0 (wc >= 123): 3, 3, 3, 4 and 5 strips, both parities of H and W
SHAPES = [(45, 245), (46, 246), (67, 364), (67, 365), (38, 487)]
# FVVDP_BAND_CR values of the sweep; None = the library's own plan
CRS = (None, 3, 4, 5, 6, 7, 9)
# display key -> the kernel variant its pooling pass takes (asserted on the GPU from the debug lines)
DISPLAYS = {"4k": 1, "hmd": 2, "custom": 3}
# the user geometry of "custom": narrow enough for its magnification (1 ... 1 / 1.375) to span at most 3 rho intervals of the CSF
# table per band, so the band's slice fits the LDS and the pass takes band_kernel<P, false, 3>
CUSTOM_GEOM = dict(distance_m=0.5, fov_diagonal=15.0)


# ------------------------------------------------------------------------------------------------------------------------------
# plan restatement (pyramid_host.hpp: band_strips, chunking; fvvdp_hip.hip: fill_band_args)
# ------------------------------------------------------------------------------------------------------------------------------
def band_strips(wc):
    return 1 if wc <= 62 else 1 + (wc - 62 + STRIP_J - 1) // STRIP_J


def chunking(hc, n_strips, n, capacity=WAVE_CAPACITY):
    """(n_chunks, cr) of a one-level launch: the chunk height that minimises rounds of resident waves x per-wave cost."""
    best, cr = 1e300, hc
    cand = 2
    while True:
        c = min(cand, hc)
        chunks = (hc + c - 1) // c
        waves = n * n_strips * chunks
        rounds = (waves + capacity - 1) // capacity
        cost = float(rounds) * (c + 8.0) * (1.0 + 1e-4 * chunks)
        if cost < best:
            best, cr = cost, c
        if cand >= hc:
            break
        cand += 1
    return (hc + cr - 1) // cr, cr


def level_sizes(W, H, n_bands):
    out = [(W, H)]
    for _ in range(n_bands):
        w, h = out[-1]
        out.append(((w + 1) // 2, (h + 1) // 2))
    return out


def plan(W, H, n_bands, n, band_cr=None, capacity=WAVE_CAPACITY):
    """[{level, n_strips, n_chunks, cr}] of the one-level launches of a W x H frame; band_cr = FVVDP_BAND_CR."""
    out = []
    sz = level_sizes(W, H, n_bands)
    for b in range(n_bands):
        wc, hc = sz[b + 1]
        ns = band_strips(wc)
        nc, cr = chunking(hc, ns, n, capacity)
        if band_cr is not None and band_cr >= 2:
            cr = min(band_cr, hc)
            nc = (hc + cr - 1) // cr
        out.append(dict(level=b, n_strips=ns, n_chunks=nc, cr=cr, hc=hc))
    return out


def chunk_lengths(hc, cr):
    """Steps of every chunk of a level: cr, ..., cr and the remainder."""
    return [min(cr, hc - ca) for ca in range(0, hc, cr)]


def row_phases(h, cr):
    """Loop phase (step<0..3> of band_item's unrolled main loop) that computes each of the h rows of a level under chunk height cr."""
    c = np.arange(h) // 2
    return (c % cr) % 4


def interior_columns(w):
    """Columns of a level that a strip which is neither the first nor the last produces: [124, 120 (n_strips - 1) + 4)."""
    ns = band_strips((w + 1) // 2)
    return 2 * (STRIP_J + 2), min(w, 2 * (STRIP_J * (ns - 1) + 2))


PLAN_RE = re.compile(r"fvvdp: level (\d+): (band_kernel<(\d), (true|false), (\d)>|multigaze_kernel<(\d), (\d)>), n (\d+), n_strips (\d+), "
                     r"n_chunks (\d+), cr (\d+), rw (\d+), lut_lds (\d)(?:, store_coarse (\d))?")


def parse_plans(err):
    """One-level launches in a captured stderr, in launch order: [{level, kernel, P, dbg, fovm | ng, n, n_strips, n_chunks, cr, rw,
    lut_lds, store_coarse}] (kernel: "band" or "multigaze")."""
    out = []
    for m in PLAN_RE.finditer(err):
        g = m.groups()
        d = dict(level=int(g[0]), n=int(g[7]), n_strips=int(g[8]), n_chunks=int(g[9]), cr=int(g[10]), rw=int(g[11]), lut_lds=int(g[12]))
        if g[1].startswith("band_kernel"):
            d.update(kernel="band", P=int(g[2]), dbg=g[3] == "true", fovm=int(g[4]))
        else:
            d.update(kernel="multigaze", P=int(g[5]), ng=int(g[6]), store_coarse=int(g[13]))
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def planar(n, P, H, W, seed):
    """Planar [n,P,H,W] fp32 in the kernels' plane order (test, reference per temporal channel).  Reference planes: positive
    luminance, every pixel independent (0.6 ... 200, as _planar of test_gpu_band2_pixels.py), so a wrong tap, row or column shows at
    its pixel.  Test planes: the reference times 1 +- 10 %, so D is neither 0 nor at its ceiling."""
    rng = np.random.RandomState(seed)
    R = np.empty((n, P, H, W), np.float32)
    for k in range(P // 2):
        ref = 0.6 + 199.4 * rng.rand(n, H, W)
        R[:, 2 * k + 1] = ref
        R[:, 2 * k] = np.clip(ref * (1.0 + 0.2 * (rng.rand(n, H, W) - 0.5)), 0.6, 200.0)
    return R


def gazes(n, H, W):
    """[n,2] (x, y) in frame pixels, per frame: inside the frame in the first interior strip of level 0, on a corner, 500 pixels
    outside, inside in the last interior strip, on the opposite corner, ...  Where the eccentricity is large the sensitivity sits
    on the floor of the CSF table and Q is pooled from the pixels around the gaze: the gazes inside are put where the walk is
    otherwise unseen.  Neighbouring frames are at least 20 pixels apart, so a wrong frame index moves every frame's Q.

    No gaze sits on a pixel centre (integer x and y): the corners are the frame's own corners, half a pixel outside the first and
    the last pixel centre.  The CSF table is indexed by sqrt(eccentricity); at the one pixel whose eccentricity is exactly 0 in
    float64, a 1e-6 degree rounding difference of the fp32 view angles moves S by 1.4e-3 (tests/test_gpu_parity.py::
    test_foveated_pq_golden bounds that pixel separately), and with Q pooled from a handful of pixels around the gaze that one
    pixel would set Q's error (measured on MI355X with the gaze on pixel (0, 0): 3.3e-3 on Q of band 0, 3e-6 on band 1)."""
    ns = band_strips((W + 1) // 2)
    assert ns >= 3                                # strip s >= 1 produces level-0 columns [120 s + 4, 120 s + 124)
    # rows of the gazes inside: coarse rows = 3 and = 2 mod 4, which chunks of 4 coarse rows compute in loop phases 3 and 2
    hc = (H + 1) // 2
    c3 = 4 * int(round((0.62 * hc - 3) / 4)) + 3
    c2 = 4 * int(round((0.24 * hc - 2) / 4)) + 2
    # (between the two fine rows of that coarse row)
    pts = [(154.0, 2 * c3 + 0.5), (-0.5, -0.5), (W + 499.0, H + 499.0), (min(120.0 * (ns - 2) + 99.0, W - 22.0), 2 * c2 + 0.5), (W - 0.5, H - 0.5)]
    fp = np.asarray([pts[i % len(pts)] for i in range(n)], np.float32)
    fp[:, 0] += np.arange(n, dtype=np.float32) // len(pts) * 23.0
    assert all(np.hypot(*(fp[i + 1] - fp[i])) >= 20.0 for i in range(n - 1))
    return fp


# ------------------------------------------------------------------------------------------------------------------------------
# the float64 yardstick
# ------------------------------------------------------------------------------------------------------------------------------
class CustomGeometry(orc.Geometry):
    """The oracle's twin of the user geometry of the GPU tests: pixels per degree falling off as 1 / (1 + angle / 20)."""

    def resolution_magnification(self, vx, vy):
        F = self.dtype
        va = np.sqrt(vx * vx + vy * vy).astype(F)
        return (F(self.ppd_centre) / (va / F(20.0) + F(1.0)) / F(self.ppd_centre)).astype(F)


def oracle(display, H, W, dtype=F64):
    """The foveated oracle of a display key (DISPLAYS) for H x W frames."""
    if display == "4k":
        return orc.Oracle("standard_4k", foveated=True, dtype=dtype)
    if display == "hmd":
        return orc.Oracle("standard_hmd", foveated=True, dtype=dtype)
    assert display == "custom"
    return orc.Oracle("standard_hmd", geometry=CustomGeometry((W, H), dtype=dtype, **CUSTOM_GEOM), foveated=True, dtype=dtype)


def reference(o, R, fixation):
    """R [n,P,H,W] through `o.process_frame`, frame by frame.  Returns dict(n_bands, rho_band, Q [bands,2,n] (channels beyond P/2
    are 0), lbkg[b] [n,h,w], contrast[b] [n,P,h,w], S[b] / D[b] [n,P/2,h,w])."""
    n, P, H, W = R.shape
    tc = P // 2
    nb, rho_band = orc.band_frequencies(W, H, o.ppd)
    out = dict(n_bands=nb, rho_band=rho_band, Q=np.zeros((nb, 2, n), o.dtype))
    per = {k: [[] for _ in range(nb)] for k in ("lbkg", "contrast", "S", "D")}
    for f in range(n):
        o.capture = {}
        out["Q"][:, :, f] = o.process_frame(f, R[f].astype(o.dtype), nb, rho_band, tc, fixation, (H, W))
        bands, lbkg = o.capture["bands"][0], o.capture["L_bkg"][0]
        for b in range(nb):
            per["lbkg"][b].append(lbkg[b])
            per["contrast"][b].append(bands[b] * o.dtype(1.0 if b == 0 else 2.0))       # the maps carry get_band's factor
            per["S"][b].append(np.stack([o.capture["S"][cc * nb + b] for cc in range(tc)], 0))
            per["D"][b].append(np.stack([o.capture["D"][cc * nb + b] for cc in range(tc)], 0))
    o.capture = None
    for k, v in per.items():
        out[k] = [np.stack(x, 0) for x in v]
    return out


def reduce64(x, times=1):
    """float64 Gaussian reduce of [P,H,W], `times` times."""
    y = np.asarray(x, F64)
    for _ in range(times):
        y = orc.gausspyr_reduce(y, F64)
    return y


def case_seed(H, W, P):
    return 1000 * H + 10 * W + P


@functools.lru_cache(maxsize=None)
def case(display, H, W, P):
    """(R [n,P,H,W] fp32, gazes [n,2], float64 reference) of one GPU case: made once, shared, never changed."""
    R = planar(N_FRAMES, P, H, W, case_seed(H, W, P))
    fp = gazes(N_FRAMES, H, W)
    ref = reference(oracle(display, H, W), R, fp)
    R.setflags(write=False)
    fp.setflags(write=False)
    return R, fp, ref


@functools.lru_cache(maxsize=None)
def discrimination(display, H, W, P):
    """What a one-row, one-column or one-frame slip of the foveated walk would do to this case, from the float64 oracle alone:
    the gaze moved by one band-0 row, by one band-0 column, and the gaze trace moved by one frame.

    Returns dict(row=, col=, frame=: |dQ| / Q [bands, P/2], S_row: mean |dS| / S [bands, P/2] under the one-row shift, the mean
    taken over every pixel of the frames whose gaze is on the screen).  A slip of the walk is in every frame and the tests bound
    every frame's Q by the same tolerance, so the frame that shows a shift most is the one that catches it: per entry the largest
    |dQ| / Q over the frames whose gaze is on the screen."""
    R, fp, ref = case(display, H, W, P)
    tc = P // 2
    on = [f for f in range(N_FRAMES) if -1 < fp[f, 0] < W and -1 < fp[f, 1] < H]
    o = oracle(display, H, W)
    out = {}
    for name, g in (("row", fp + np.float32([0, 1])), ("col", fp + np.float32([1, 0])), ("frame", np.roll(fp, 1, axis=0))):
        alt = reference(o, R, g)
        dq = np.abs(alt["Q"] - ref["Q"]) / ref["Q"][:, :, :].clip(1e-300)
        out[name] = np.max(dq[:, :tc][:, :, on], axis=2)
        if name == "row":
            out["S_row"] = np.array([[np.mean(np.abs(alt["S"][b][on, cc] - ref["S"][b][on, cc]) / ref["S"][b][on, cc]) for cc in range(tc)]
                                     for b in range(ref["n_bands"])])
    return out
