#!/usr/bin/env python3
"""Turn gpurun_out/prof_bundle/ (written by tools/collect_profiles.sh on the GPU box, ONE gpurun call = one box) into the
tracked files profiles/<round>_final_kernel_trace.md, profiles/<round>_pmc_level0.json, profiles/<round>_parity_stages.md (round 6 on: `<round>_parity.md` is a separate evidence file).
usage: make_profile_doc.py r02"""
import json, os, shutil, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = os.path.join(ROOT, "gpurun_out", "prof_bundle")
tag = sys.argv[1] if len(sys.argv) > 1 else "r03"
rd = lambda n: open(os.path.join(B, n)).read().strip() if os.path.exists(os.path.join(B, n)) else "(not collected)"


def kt(name):
    return "\n".join(l for l in rd(name).split("\n")
                     if (l.startswith("|") and ("temporal_" in l or "band_kernel" in l or "band2_kernel" in l or "finalize" in l or "pool_jod" in l
                                                or "band_tail" in l or l.startswith("| kernel") or l.startswith("|---"))))


def dispatch_list(name):
    txt = rd(name)
    i = txt.find("dispatches of")
    return txt[i:] if i >= 0 else "(no dispatch list)"


def same_box_table():
    """rocprof per-launch figures next to the HIP-event figures of the SAME profiled process."""
    try:
        j = json.loads(rd("bench_profiled.json").split("\n")[-1])
    except Exception:
        return "(bench_profiled.json not collected)"
    rows = {}
    for l in rd("kernel_trace_bench.md").split("\n"):
        c = [x.strip() for x in l.split("|")]
        if len(c) > 8 and ("band" in c[1] or "finalize" in c[1]) and c[2].isdigit():
            rows[c[1]] = (int(c[2]), float(c[4]), float(c[5]), float(c[6]), float(c[7]))       # calls, avg, median, steady median, min
    g = j["graded_pass"]
    n = j["roofline"]["frames_per_launch"]
    alg = g["algorithmic_bytes_per_frame"]
    out = ["| kernel (rocprofv3 label) | rocprof avg us / launch | rocprof median | steady median (first 3 dropped) | min | per frame (steady median) | HIP events, median per frame |", "|---|---|---|---|---|---|---|"]
    tot = {"avg": 0.0, "med": 0.0, "steady": 0.0, "min": 0.0}
    ev = list(g["levels_us_per_frame_median"]) + [g["finalize_us_per_frame"]]
    for label, (calls, avg, med, steady, mn) in sorted(rows.items(), key=lambda kv: kv[0].split("[")[-1] if "[" in kv[0] else "z"):
        e = ""
        if "levels 0+1" in label: e = "%.2f" % ev[0]
        elif "[level " in label: e = "%.2f" % ev[int(label.split("[level ")[1].split("]")[0])]
        elif "finalize" in label: e = "%.2f" % ev[-1]
        out.append("| %s | %.1f | %.1f | %.1f | %.1f | %.2f | %s |" % (label, avg, med, steady, mn, steady / n, e))
        tot["avg"] += avg / n; tot["med"] += med / n; tot["steady"] += steady / n; tot["min"] += mn / n
    out.append("| **all pyramid levels + finalize (graded pass)** | %.2f / frame | %.2f | **%.2f** | %.2f | | **%.2f** (min %.2f) |" % (
        tot["avg"], tot["med"], tot["steady"], tot["min"], g["us_per_frame_all_levels"], g["us_per_frame_all_levels_min"]))
    out.append("")
    fr = lambda us: alg / (us * 1e-6) / 8e12
    out.append("Graded pass against SURVEY 8(d)'s %.1f MB per frame and the 8 TB/s spec peak: **%.3f from the rocprof steady medians, %.3f from "
               "the rocprof medians over all launches, %.3f from the rocprof averages (they include the cold launches listed below), %.3f from "
               "the HIP-event medians** of the same process (target >= 0.60, i.e. <= 46.1 us per frame)." % (
                   alg / 1e6, fr(tot["steady"]), fr(tot["med"]), fr(tot["avg"]), g["hbm_frac_all_levels"]))
    r = j["roofline"]
    for label, (calls, avg, med, steady, mn) in rows.items():
        if "levels 0+1" in label:
            out.append("")
            out.append("Dominant kernel (`roofline` of the JSON line): algorithmic %.4f GB per launch / rocprof steady median %.1f us = %.0f GB/s = "
                       "**%.3f**; / HIP-event median %.1f us = %.0f GB/s = **%.3f** (difference %.1f %%).  With the bytes it really moves "
                       "(PMC, %s): %.0f GB/s = %.3f of the peak." % (
                           r["bytes_per_launch"] / 1e9, steady, r["bytes_per_launch"] / steady / 1e3, r["bytes_per_launch"] / steady / 1e3 / 8000.0,
                           r["median_launch_ms"] * 1e3, r["achieved"], r["frac"], 100.0 * abs(steady - r["median_launch_ms"] * 1e3) / steady,
                           "live" if r.get("traffic") else "not collected", (r.get("achieved_traffic") or 0.0), (r.get("frac_traffic") or 0.0)))
    return "\n".join(out)


def quoted_figures():
    """The derived figures DESIGN.md section 0 quotes, computed here from the files of the bundle so that they are grep-able."""
    try:
        jp = json.loads(rd("bench_plain.json").split("\n")[-1])
        jq = json.loads(rd("bench_profiled.json").split("\n")[-1])
    except Exception:
        return "(bench lines not collected)"
    rows = {}
    for l in rd("kernel_trace_bench.md").split("\n"):
        c = [x.strip() for x in l.split("|")]
        if len(c) > 8 and c[2].isdigit():
            rows[c[1]] = (int(c[2]), float(c[4]), float(c[5]), float(c[6]))       # calls, avg, median, steady
    out = []
    r, k1, g = jp["roofline"], jp["roofline_k1"], jp["graded_pass"]
    out.append("* unprofiled `bench.py`: %.3f ms per pair = %.1f Gpix/s (test+ref), median of %d steps (mean %.3f, min %.3f, max %.3f); profiled: %.3f ms" % (
        jp["ms_per_step"], jp["value"] / 1e3, jp["steps"], jp["timing"]["ms_per_step_mean"], jp["timing"]["ms_per_step_min"], jp["timing"]["ms_per_step_max"], jq["ms_per_step"]))
    for label, (calls, avg, med, steady) in rows.items():
        if "band2_kernel" in label and "levels 0+1" in label:
            b = r["bytes_per_launch"]
            if "false" in label and jp["roofline"]["kernel"].startswith("band2_kernel<4, true>"):
                out.append("* `%s`: %d launches, rocprof AVERAGE %.1f us -- not the timed steps: the `roofline.with_clamps` leg of bench.py (the same launch with the four clamps "
                           "kept, a second context, its first touch included)" % (label.strip("`"), calls, avg))
                continue
            out.append("* `%s`: %.4f GB algorithmic per launch / rocprof AVERAGE %.1f us = %.2f TB/s = %.3f of 8 TB/s; / steady median %.1f us = %.3f; unprofiled HIP-event median %.1f us = %.4f" % (
                label.strip("`"), b / 1e9, avg, b / avg / 1e6, b / avg / 1e6 / 8.0, steady, b / steady / 1e6 / 8.0, r["median_launch_ms"] * 1e3, r["frac"]))
        if "temporal_vec_kernel" in label:
            b = k1["bytes_per_launch"]
            n = k1["frames_per_launch"]
            out.append("* `%s`: %.1f MB per frame; %d launches, rocprof AVERAGE %.1f us per %d frames = %.1f us per frame = %.2f TB/s = %.3f (all launches of the process, the first touch of a fresh context included); rocprof MEDIAN %.1f us = %.1f us per frame = %.3f; "
                       "unprofiled HIP events %.2f us per frame = %.4f" % (
                label.strip("`"), b / n / 1e6, calls, avg, n, avg / n, b / avg / 1e6, b / avg / 1e6 / 8.0, med, med / n, b / med / 1e6 / 8.0,
                g["temporal_us_per_frame_median"], k1["frac"]))
    if r.get("frac_rocprof_avg"):
        out.append("* `roofline` of the unprofiled line: frac %.4f (HIP-event median), frac_rocprof_avg %.4f (kernel trace run from bench.py, %.4f ms average), frac_bmin %.4f; "
                   "with_clamps (`band2_kernel<4, false>`): %s" % (r["frac"], r["frac_rocprof_avg"], r.get("rocprof_avg_launch_ms", 0), r.get("frac_bmin", 0),
                                                                      ("frac %.4f, all levels %.2f us per frame" % (r["with_clamps"]["frac"], r["with_clamps"]["us_per_frame_all_levels"])) if r.get("with_clamps") else "-"))
    if jp.get("collective"):
        out.append("* one-rank collective of the unprofiled line: %s, %.1f us per call back to back (RCCL %s)" % (
            jp["collective"].get("backend"), jp["collective"].get("us_per_call_back_to_back", 0), (jp.get("communicator") or {}).get("rccl_version")))
    try:
        j3 = json.loads(rd("bench_config3.json").split("\n")[-1])
        rf = j3["roofline_fov"]
        out.append("* `bench.py --config 3` (3840x2160 x120 foveated, PQ): %.3f ms per pair = %.1f Gpix/s; roofline_fov: levels %s us per frame, all levels %.2f = %.4f of the peak "
                   "(target 0.60 = %.2f us), frac_bmin %.4f; JOD delta to the reference %.3g" % (j3["ms_per_step"], j3["value"] / 1e3, rf["us_per_frame_levels"], rf["us_per_frame_all_levels"],
                                                                                                   rf["frac"], rf["target_us_per_frame"], rf["frac_bmin"], j3.get("jod_delta_vs_reference") or 0.0))
    except Exception:
        pass
    if r.get("traffic"):
        out.append("* real traffic of the dominant kernel: %.2f GB per launch = %.3f of the algorithmic bytes; %.2f TB/s = %.3f of the peak" % (
            r["traffic"] / 1e9, r["traffic_over_algorithmic"], r["achieved_traffic"] / 1e3, r["frac_traffic"]))
    out.append("* graded pass, unprofiled: %.1f us per frame = %.3f; profiled HIP events %.2f us = %.3f" % (
        g["us_per_frame_all_levels"], g["hbm_frac_all_levels"], jq["graded_pass"]["us_per_frame_all_levels"], jq["graded_pass"]["hbm_frac_all_levels"]))
    rs = jp["roofline_step"]
    out.append("* whole step: %.2f GB per pair, %.2f TB/s = %.3f; kernels back to back %.3f ms of %.3f ms" % (
        rs["bytes_per_step"] / 1e9, rs["achieved"] / 1e3, rs["frac"], rs["kernels_back_to_back_ms"], rs["ms_per_step"]))
    for name in ("bench_malloc.json", "bench_chunks.json", "bench_clamps.json", "bench_noticket.json", "bench_pairs8.json", "bench_frames.json",
                 "bench_fhd.json", "bench_fhd_plain.json", "bench_collective_off.json", "bench_collective_force.json"):
        try:
            j = json.loads(rd(name).split("\n")[-1])
            gg = j["graded_pass"]
            out.append("* `%s`: %.3f ms per pair = %.1f Gpix/s; K1 %.2f us, levels 0+1 %.2f us, all levels %.2f us per frame" % (
                name, j["ms_per_pair"], j["value"] / 1e3, gg["temporal_us_per_frame_median"], gg["levels_us_per_frame_median"][0], gg["us_per_frame_all_levels"]))
        except Exception:
            pass
    la = jp.get("level0_alloc")
    if isinstance(la, dict):
        pr = la.get("pair_write_rate_tbs") or {}
        out.append("* level 0 of the unprofiled run: %s%s; host syncs / allocations / frees inside per-frame calls: %s; first step incl. context creation %s ms" % (
            la.get("in_use"),
            (" (fvvdp_ctx_create wrote every pair of %s half-size candidates at once: %.2f TB/s for the pair kept, %.2f for the slowest)" % (
                la.get("half_size_candidates"), pr.get("kept", 0), pr.get("lowest", 0)))
            if la.get("half_size_candidates") else "",
            "/".join(str(v) for v in (la.get("per_frame_calls") or {}).values()), la.get("first_step_ms_incl_context_creation")))
    if jp.get("predict_call_ms"):
        out.append("* step path: %s; the reference-style synchronous `predict()` on the same pair: %.3f ms" % (jp.get("step_path"), jp["predict_call_ms"]))
    if k1.get("traffic"):
        out.append("* real traffic of the temporal kernel: %.2f GB per launch = %.3f of its algorithmic %.2f GB (the excess is the 7 history frames)" % (
            k1["traffic"] / 1e9, k1.get("traffic_over_algorithmic", 0), k1["bytes_per_launch"] / 1e9))
    out.append("* JOD %s, |delta| to the real reference %.3g (north-star bound 1e-3)" % (jp.get("jod"), jp.get("jod_delta_vs_reference") or 0.0))
    fov = [l for l in rd("fov_probe.txt").split("\n") if l.startswith("kernel us/frame")]
    fms = [l.split()[4] for l in rd("fov_probe.txt").split("\n") if l.startswith("config4")]
    if fov:
        out.append("* configs[3] (3840x2160 x120 foveated, moving gaze, PQ; `fov_probe.txt`): calls %s ms; %s" % (" / ".join(fms[1:]), fov[0]))
        if len(fov) > 1:
            out.append("  %s" % fov[1])
    cb = jp.get("cpu_baseline") or {}
    if cb:
        out.append("* CPU baseline: %.2f Mpix/s on %d cores; reference %.1f s per pair = %.2f Mpix/s; PCIe-inclusive %.1f Gpix/s" % (
            cb["value"], cb["cores"], cb.get("reference_torch_cpu_seconds_build_container", 0), cb.get("reference_torch_cpu_mpix_s_build_container", 0),
            jp.get("value_h2d_inclusive", 0) / 1e3))
    return "\n".join(out)


doc = f"""# Round {tag[1:]} -- rocprofv3 --kernel-trace --stats of `python bench.py --no-cpu-baseline` (final build of the round)

Produced by `tools/collect_profiles.sh` in ONE gpurun call (one box) and formatted by `tools/make_profile_doc.py`.
Workload: 3840x2160 x60 uint8 RGB pair, standard_4k, 30 fps (8 taps), non-foveated; 5 warm-up + 10 timed steps + the
in-library HIP-event timing pass (>= 10 further calls, kernels strictly one after the other) + the host-array call.  band_kernel rows are labelled by pyramid
level (dispatch order); `band2_kernel` covers two levels per launch.  torch kernels of the synthetic input generator
(setup, untimed) are omitted.

{kt('kernel_trace_bench.md')}

Figures derived from this bundle (quoted in DESIGN.md section 0):

{quoted_figures()}

Every launch of the dominant kernel in that process, in order, with the kernel that ran before it.  The launches behind
`__amd_rocclr_copyBuffer` are the host-array (PCIe-inclusive) calls at the end of bench.py: the GPU idles during the 50 ms
upload and the kernel starts on cold clocks.  After every idle gap the launches of this arithmetic-bound kernel come down over
the first 6-8 launches (~30 ms: 2.5 -> 2.3 -> 2.2 -> 2.0 -> 1.94 -> 1.89 -> 1.85 ms) while the power controller brings the clocks up
(`profiles/r05_power.md`: the steady state sits at 1350 W of 1400, sclk 2.1 GHz); those launches are what separates the rocprof AVERAGE
from the steady median and from the HIP-event median of the timed steps (bench.py warms up for 10 steps by default for this reason):

```
{dispatch_list('kernel_trace_bench.md')}
```

## The graded pass on ONE box: rocprof next to the in-library HIP events

{same_box_table()}

## What bounds the dominant kernel: SQ / TCC counters (separate --pmc passes of `tools/gpu_bandonly.py`)

`tools/pmc_sq_summary.py`; shares are of the waves' resident time (SQ_WAVE_CYCLES).  Read together with the ablation builds
(`profiles/r04_pyramid_kernel.md`: arithmetic alone 28.7-28.9 us per frame, data flow alone 32.2-32.3 us, together 35.1-35.6 us on one box):
the kernel is co-bound, since round 4 (clamp-free variant) with the data flow as the longer of the two floors.

{rd('pmc_sq_bandonly.md')}

The foveated kernel (`tools/gpu_fov_bandonly.py`; levels 0 and 1 share a grid size and are averaged in the first block):

{rd('pmc_sq_fov_bandonly.md')}

## Registers, spills, scratch of every kernel in the shipped library (code-object metadata, `tools/codeobj_report.py`)

{rd('codeobj.md')}

bench.py JSON of the SAME profiled process (HIP events on the kernels' stream):

```
{rd('bench_profiled.json')}
```

bench.py JSON of the unprofiled run on the same box, right before:

```
{rd('bench_plain.json')}
```

`--pairs-per-gpu 8` (BASELINE configs[4] per GPU: 8 pairs queued without host synchronisation), same box:

```
{rd('bench_pairs8.json')}
```

Same box, one switch at a time: the level-0 buffer fixed to one kind and no comparison at creation (`FVVDP_ALLOC=malloc
FVVDP_PLACEMENT_PROBE=0`, then `FVVDP_PLACEMENT_PROBE=0` = 32 MB chunks; the default line above keeps the fastest of four candidates,
`level0_alloc` says which: `profiles/r05_k1_mode.md`), `FVVDP_BAND_INRANGE=0` (the pyramid kernel with its clamps) and
`FVVDP_BAND2_TICKET=0` (static split of the pyramid kernel's work items, `profiles/r05_band2_tickets.md`):

```
{rd('bench_malloc.json')}
{rd('bench_chunks.json')}
{rd('bench_clamps.json')}
{rd('bench_noticket.json')}
```

`--shard frames` on one rank (the frame-sharded step path: `predict_frame_sharded`, all-reduce skipped), same box:

```
{rd('bench_frames.json')}
```

## BASELINE configs[1]: 1920x1080 x60, standard_fhd (6 bands) -- kernel table of `bench.py --width 1920 --height 1080 --display standard_fhd`

{kt('kernel_trace_fhd.md')}

The profiled line and the unprofiled one of the same box:

```
{rd('bench_fhd.json')}
{rd('bench_fhd_plain.json')}
```

Per pixel the 1080p pair is slower than the 4K pair ONLY in the pyramid pass (the temporal kernel scales with the pixel count:
compare its us per frame x 4 with the 4K table).  The two-level kernel covers a 1080p frame with 18 strips x 8 chunks of 34 level-C rows
(cost model of `chunking2`): 8640 single-wave workgroups for 60 frames = 2.8 rounds of the 3072 resident waves, and every chunk
pays 9 halo steps on top of its 68 (13 %; 4K: 78-row chunks, 9 on 156 = 6 %, 4.9 rounds); the launch lasts 0.6 ms, so ramp-up and
drain (~25 us) weigh 4 % where they weigh 1 % at 4K; the small levels (2..5) and the finalisation are launch-latency-sized at both
resolutions and therefore four times as heavy per pixel at 1080p.

## A/B on the same box: two levels per pass (band2_kernel) vs one level per pass (FVVDP_BAND_FUSE=0)

Stage 2 alone on resident level-0 data (`tools/gpu_bandonly_speed.py`, HIP events, 12 calls each):

```
{rd('bandonly_fused.txt')}
{rd('bandonly_onelevel.txt')}
```

Kernel trace of `FVVDP_BAND_FUSE=0 python bench.py` (the round-1 structure, same box):

{kt('kernel_trace_bench_onelevel.md')}

## HBM traffic of the dominant kernel (separate `--pmc` passes, `tools/gpu_bandonly.py`)

`profiles/{tag}_pmc_level0.json` (same call): FETCH_SIZE x2 + WRITE_SIZE per launch.  `algorithmic_bytes` is SURVEY 8(d)'s
streaming-pyramid figure for the levels the launch covers; the two-level kernel moves LESS than that (level 1 never leaves
the chip): `compulsory_bytes_of_this_kernel` is what it has to move, the excess over it is the strip halo (20 of 128 columns).

```
{rd('pmc_level0.json')}
```

The one-level kernel at level 0 (FVVDP_BAND_FUSE=0), same counters:

```
{rd('pmc_level0_onelevel.json')}
```

Why two levels per pass: any mix of reads and writes tops out near 4.9-5.0 TB/s on this memory system, pure reads reach
6.1-6.3 (`tools/microbench/mix.hip`, same box) -- the one-level kernel's 4:1 mix was at that ceiling:

```
{rd('mix.txt')}
```

K1 (`temporal_vec_kernel<8,4,0>`), same counters over whole `predict` calls (KiB per dispatch).  Algorithmic per 60-frame
launch: 60 x 132.7 MB = 7.96 GB written; 67 source frames x 49.8 MB = 3.33 GB read (the raw FETCH_SIZE scale for these
4 B/lane loads is ~2.2, not the 2.0 calibrated for 16 B/lane streaming reads):

```
{rd('pmc_k1.txt')}
```

## Other frame rates and input types, frame sources (same call)

`tools/gpu_fps.py` (4K; K1 = temporal kernel per frame, HIP events, mean of 4 calls incl. the first) and `tools/gpu_k1_ab.py`
(median over fresh allocations, warm-up call dropped):

```
{rd('fps_probe.txt')}
```

K1 at 60 / 120 fps and for uint16 input under rocprofv3 (`tools/gpu_fps.py 60:120:u8 120:120:u8 30:60:u16`; one launch = 120 / 120 / 60
output frames, 4 calls each):

{rd('kernel_trace_rates.md')}

`tools/gpu_feeder.py` (1080p x60, then 4K x60; user video sources through their own get_*_frame, SURVEY 8(f) rank 3):

```
{rd('feeder_probe.txt')}
```

## "Next"-row kernels (SURVEY section 8(f)) and the foveated configuration, same call

YUV ingest (`tools/gpu_yuv.py`: 4K x60, 4:2:0 8 bit 30 fps / 4:2:0 10 bit 60 fps / 4:4:4 8 bit 30 fps; one launch = 60 output frames):

{rd('kernel_trace_yuv.md')}

```
{rd('yuv_probe.txt')}
```

PU21-PSNR (`tools/gpu_psnr.py`: 4K x60 uint8, 4K x20 fp32):

{rd('kernel_trace_psnr.md')}

```
{rd('psnr_probe.txt')}
```

Coloured heat maps (`tools/gpu_heatprof.py 12 threshold`: 4K, 12 frames in batches of 5; `band_kernel<4, true, 0>` is
the map-writing variant of the pyramid kernel):

{rd('kernel_trace_heat.md')}

```
{rd('heat_probe.txt')}
```

BASELINE configs[3] (`tools/gpu_config4.py`: 4K x120, foveated, moving gaze, PQ display; `band_kernel<4, false, 1>` is the
foveated variant with the band's LUT slice in LDS; `fov_rho_map_kernel` runs once per geometry):

{rd('kernel_trace_fov.md')}

```
{rd('fov_probe.txt')}
```
"""
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
open(os.path.join(ROOT, "profiles", f"{tag}_final_kernel_trace.md"), "w").write(doc)
for src, dst in (("pmc_level0.json", f"{tag}_pmc_level0.json"), ("pmc_level0_onelevel.json", f"{tag}_pmc_level0_onelevel.json")):
    if os.path.exists(os.path.join(B, src)):
        shutil.copy(os.path.join(B, src), os.path.join(ROOT, "profiles", dst))
if os.path.exists(os.path.join(B, "parity.md")):
    par = f"""# Round {tag[1:]} -- measured parity of the HIP path on MI355X, stage by stage

Written by `tools/gpu_parity_report.py` (inside `tools/collect_profiles.sh`).  Goldens = captures of the real reference
(`tools/gen_golden.py`, tests/golden/); "oracle" = `oracle/fvvdp_oracle.py`.  The bounds asserted in `tests/` are <= 3x the
numbers below (each bound quotes its measured value).  JOD: north-star bound 1e-3.

{rd('parity.md')}

End to end against the goldens g9 (120 / 144 / 240 fps; uint8, uint16, float RGB behind PQ, float gray) g10 (the other
eleven display models, plain and foveated) g11 (caller-built photometry / geometry objects) and g12 (foveated heat maps), `tools/gpu_g9_report.py` /
`gpu_g10_report.py` / `gpu_g11_report.py`; dQ = max |Q - Q_ref| / (|Q_ref| + 1e-3 max Q_ref):

```
{rd('parity_goldens.txt')}
```

Notes.
* `D per pixel`: relative to |D| + 1e-3 max(D); the maxima are single pixels whose contrast is ~1 ulp of the Gaussian
  levels (D ~ contrast^2.4 amplifies it), the means are what the pooled sums see.
* Foveated mode: the spread against the reference (S up to 1.1e-2) is the reference's own rounding noise -- its resolution
  magnification is a finite difference of fp32 tangents (fvvdp_display_model.py:475-488).  The same formula with fp64
  geometry (`Geometry.exact_geometry`, tests only) is as far from the reference as the kernel is, and agrees with the kernel
  ~10x better (end to end 1.3e-4 on Q_per_ch, 2e-6 on JOD).  The remaining 1.3e-3 maximum on S is the single pixel under the
  gaze, where sqrt(ecc) amplifies a 1e-6 deg rounding difference of the eccentricity.
"""
    open(os.path.join(ROOT, "profiles", f"{tag}_parity_stages.md"), "w").write(par)
print("wrote profiles/%s_final_kernel_trace.md (%d bytes)" % (tag, len(doc)))
# DESIGN.md section 0 quotes exactly these figures: splice them in between the markers
dpath = os.path.join(ROOT, "DESIGN.md")
if os.path.exists(dpath):
    d = open(dpath).read()
    b, e = "<!-- bundle-figures:begin -->", "<!-- bundle-figures:end -->"
    if b in d and e in d:
        d = d[:d.index(b) + len(b)] + "\n" + quoted_figures() + "\n" + d[d.index(e):]
        open(dpath, "w").write(d)
        print("updated the figures block of DESIGN.md")

