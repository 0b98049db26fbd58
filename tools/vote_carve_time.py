#!/usr/bin/env python3
"""The vote carve (arvx_carve_votes) against the plain carve on the 512^3 sphere scene, 36 views of
640x480, a fresh model every time.  Five legs, WARMUP + REPS calls each, one after the other:

    1. arvx_carve, default flags (the three-launch carve)
    2. arvx_carve with ARVX_CARVE_NO_CULL (the brute-force carve_fused_kernel)
    3. arvx_carve_votes, max_misses = 0
    4. arvx_carve_votes, max_misses = 2
    5. arvx_carve_votes, max_misses = 2, ARVX_VOTES_COUNTS

Run it under the profiler, then let it read the trace (GPU required for the first command):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/vote_carve_time.py [N]
    python tools/vote_carve_time.py --summarize OUT

The first prints, per leg, the median of the calls' host time up to a synchronisation (which holds
the launch overhead: about as much as the shorter legs' kernels).  The second prints the five
KERNEL-time medians from the trace: a call's time is the sum of the carve kernels it launched, the
legs are told apart by the kernels' names and their order, and the warm-up calls are left out.  The
one condition DESIGN 4.9 sets is checked there: leg 3 must not be slower than leg 2."""
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V = 36
WARMUP = 3
REPS = 21
LEGS = ("arvx_carve", "arvx_carve NO_CULL", "arvx_carve_votes K=0", "arvx_carve_votes K=2",
        "arvx_carve_votes K=2 COUNTS")


def run(N):
    from ar_voxel_project_amd import capi, synthetic
    capi.load_library()
    sc = synthetic.sphere_scene(N, V)
    with capi.Context(N, N, N, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, sc.masks)
        legs = (lambda: ctx.carve(), lambda: ctx.carve(capi.CARVE_NO_CULL), lambda: ctx.carve_votes(0),
                lambda: ctx.carve_votes(2), lambda: ctx.carve_votes(2, counts=True))
        occupied = []
        print(f"{N}^3, {V} views of {sc.W}x{sc.H}, fresh model; host time of a call up to a synchronisation, "
              f"median of {REPS}:")
        for name, leg in zip(LEGS, legs):
            t = []
            for i in range(WARMUP + REPS):
                ctx.reset()
                ctx.synchronize()
                t0 = time.perf_counter()
                leg()
                ctx.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            occupied.append(int((ctx.download_state() & 1).sum()))
            print(f"  {name:30s} {np.median(t[WARMUP:]):8.3f} ms   occupied {occupied[-1]}")
        assert occupied[0] == occupied[1] == occupied[2], "max_misses = 0 is the carve"
        assert occupied[3] == occupied[4] >= occupied[2]


def summarize(out_dir):
    traces = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not traces:
        sys.exit(f"no *kernel_trace.csv under {out_dir}")
    rows = []
    for path in traces:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    calls = [[] for _ in LEGS]  # per leg: kernel nanoseconds of each call
    votes = 0
    for start, end, name in rows:
        if "carve_votes_kernel" in name:
            leg = 2 + votes // (WARMUP + REPS)
            votes += 1
            if leg < len(LEGS):
                calls[leg].append(end - start)
        elif "carve_fused_kernel" in name:
            calls[1].append(end - start)
        elif "carve_coarse_kernel" in name:  # the first launch of a default carve
            calls[0].append(end - start)
        elif "arvx::carve_" in name or "carve_classify" in name or "carve_exact" in name:
            if calls[0]:
                calls[0][-1] += end - start
    med = []
    print(f"kernel time per call from {len(traces)} trace file(s), median of {REPS} (after {WARMUP} warm-up calls):")
    for name, c in zip(LEGS, calls):
        if len(c) != WARMUP + REPS:
            sys.exit(f"{name}: {len(c)} calls in the trace, expected {WARMUP + REPS}")
        med.append(float(np.median(c[WARMUP:])) / 1e6)
        print(f"  {name:30s} {med[-1]:8.4f} ms   (min {min(c[WARMUP:]) / 1e6:.4f}, max {max(c[WARMUP:]) / 1e6:.4f})")
    print(f"vote carve K=0 / brute-force carve: {med[2] / med[1]:.3f}   (the condition: <= 1)")
    print(f"vote carve K=0 / default carve:     {med[2] / med[0]:.2f}")
    print(f"counts on top of K=2:               {med[4] / med[3]:.2f}")
    if med[2] > med[1]:
        sys.exit("the culled vote carve at max_misses = 0 is SLOWER than the brute-force carve: its culling is not working")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
