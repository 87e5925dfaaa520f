#!/usr/bin/env python3
"""Isolated-operator benchmark, the counterpart of the reference's tests/performance/perf_cuda_tridiag.f90 and
perf_cuda_transeq.f90: tds_solve with the periodic compact6 second derivative and the
fused transport-equation component on 512^2 pencils of n points, input sin(j dx) as there, n_warmup untimed +
n_iters timed launches.  Prints one JSON line per case: achieved GB/s on ALGORITHMIC bytes
(tds_solve 16 B/DoF, transeq component 24 B/DoF, 16 when conv = u) and the reference's own convention
(the "consumed bandwidth" its perf tests assume: 6 passes = 48 B for tds_solve, 16 passes = 128 B for transeq).

    python bench_ops.py [--n 256,512,1024] [--iters 50] [--family all|operators|stats|ibm|snapshot|checkpoint|spectra|diagnostics|budgets|loads|les|particles|scalars|forcing|feedback]

Family "statistics sample" (n^3 grids, n = 256 and 512; HIP-event time per launch group, median of --stat-iters after
--stat-warmup): the fused 3-D update (x3d_stats_update_uvw, 168 B/DoF in FP64), the profile update along y
(x3d_stats_profile_sums + _accumulate, 24 B/DoF), the same nine running means composed from veccopy / vecmult / vecadd
(456 B/DoF: what the entry points of the reference's backend interface cost), and the existing reduction
x3d_scalar_product on the same field (16 B/DoF).  GB/s on those stated bytes; `ceiling` = fraction of the 6.2 TB/s copy
ceiling (profiles/r04_copy_ceiling.txt).

Family "ibm" (FP64, HIP-event time, median of --stat-iters): on a 512^3 periodic block with a cylinder of diameter
L_x / 20 along z, (a) Ibm.body through the work list against one and three x3d_vecmult by a device mask; (b) the
cylinder case's per-sub-step boundary path, x3d_outflow_params + x3d_cylinder_apply_bc + Ibm.body, against the calls
of the reference composed (three slice_max_sum, three field_set_face_from_field, three vecmult), with the number of host
waits for the stream in each (x3d_backend_counter 3); (c) make_cylinder((257, 128, 32)), 20 steps, ms per step with the
work list and with X3D_NO_IBM_SPARSE=1.  `step_share` = fraction of the 40 ms of a 512^3 TGV step (README).

Family "snapshot" (FP64, --snap-n^3 = 512^3, median of --stat-iters; not part of "all"): (a) the pack kernel with six
variables (u, v, w, p, vort, qcrit) at strides (1,1,1) and (2,2,2), 4- and 8-byte output: HIP-event ms and GB/s on
touched source lines plus output bytes (a 128-byte line counts whole when one of its points is kept), next to the
6.2 TB/s copy ceiling; (b) host-visible time of Snapshots.write from call to return against the composed path in the
same process (six get_field_data, two compute_*, numpy striding and astype); (c) a 20-step TGV run at snapshot_freq = 5
against the same run without snapshots: added wall time per snapshot.

Family "checkpoint" (--snap-n^3 = 512^3, median of --stat-iters; not part of "all"): (a) the pack launch with its checksums
for 3 and for 12 blocks against the 6.2 TB/s copy ceiling; (b) Checkpoints.write from call to return against get_field_data
of the same 12 blocks; (c) a 20-step TGV run at checkpoint_freq = 5 against the same run without checkpoints, and the time
poll() spent writing files on the host thread.

Family "spectra" (--snap-n^3 = 512^3, HIP-event time, median of --stat-iters; not part of "all"): (a) the shell-binning
launches alone (x3d_spectra_reduce) against the bytes they must read, nz ny nxs complex numbers, and the 6.2 TB/s copy
ceiling, next to x3d_scalar_product on a field of the same run; (b) a whole three-field sample, three forward transforms
plus three reductions plus the running-mean update; (c) the composed path in the same process, get_spectral plus numpy
binning for three fields (wall clock: it waits for the host); (d) the plane reduction alone and a three-field plane sample
at 1024 x 257 x 512.  `step_share` = fraction of the 40 ms of a 512^3 TGV step (README).

Family "diagnostics" (--snap-n^3 = 512^3, median of --stat-iters with the quartiles as spread; not part of "all"): (a) the
x3d_diag_reduce launches alone (HIP events) in GB/s on the twelve blocks they must read, next to the 6.2 TB/s copy ceiling
and x3d_scalar_product on the same box; (b) a whole Diagnostics sample -- nine gradients, the reduction, the divergence and
its max / sum -- as wall clock around a device sync; (c) Monitoring.write_step + kinetic_energy on the same state in the
same process, the same way, with the host waits of each (x3d_backend_counter 3); (d) a 20-step TGV run with idiagfreq = 1
against the same run without: added wall time per step.  The lines are appended to profiles/diagnostics.jsonl.

Family "budgets" (--snap-n^3 = 512^3, median of --stat-iters with the quartiles as spread; not part of "all"): (a) the
x3d_budget_profile_sums launches alone (HIP events) in GB/s on the thirteen blocks they read (104 B/DoF in FP64), next to
x3d_diag_reduce (96 B/DoF) in the same process, and the gate t_budget <= 1.25 (104 / 96) t_diag_reduce; (b) a whole
Budgets.update as wall clock around a device sync; (c) the composed host path in the same process, thirteen get_field_data
plus numpy moments; (d) a 20-step TGV run with ibudfreq = 1, pressure = False against the same run without: added wall time
per step.  The lines are appended to profiles/budgets.jsonl.

Family "loads" (median of --stat-iters with the quartiles as spread; not part of "all"): on a 512 x 256 x 64 box with the
default cylinder's proportions (20 x 12 x 6, diameter 1 through (L_x / 4, L_y / 2)), (a) x3d_ibm_body_loads, both launches,
next to x3d_ibm_body on the same work list (HIP events), and how far the first lies above the second; (b) x3d_probe_sample
for 256 probes; (c) 20 steps of make_cylinder((257, 128, 32), fused=True) with Loads at every step against the same run
without, and (d) the same with Loads and Probes: wall time, the host waits (x3d_backend_counter 3) of each run during the
steps and in finalise, and the launch groups of the per-class timers per sub-step (taken in a second, untimed run of 5 steps;
with Loads they grow by exactly one, the finishing launch).  No gate on the times; the two counts are gates.  The lines are
appended to profiles/loads.jsonl.

Family "les" (--snap-n^3 = 512^3, median of --stat-iters with the quartiles as spread; not part of "all"): (a) x3d_les_stress,
both launches (HIP events), for both models, in TB/s on the 128 B/DoF it reads and writes in FP64 (the nine gradients are
restored before every timed call: the kernel works in place), next to the fused statistics update (168 B/DoF, also a read +
write stream) in the same process, and the gate t_stress <= 1.25 (128 / 168) t_stats_update; (b) a whole Les.add next to a
whole Diagnostics sample, wall clock around a device sync; (c) 20 fused RK3 TGV steps with and without the model: added wall
time per step (no gate); (d) x3d_les_scalar_flux (the species' subgrid flux; 56 B/DoF for one species, 104 B/DoF for two in
FP64) with the fused statistics update timed in the same loop, and the gates t_flux <= 1.25 (56 / 168) t_stats_update and
1.25 (104 / 168); (e) a whole Les.add with one species; (f) 20 fused RK3 TGV steps with LES alone, with one species alone and
with both (no gate).  The lines are appended to profiles/les.jsonl.

Family "particles" (--snap-n^3 = 512^3, median of --stat-iters with the quartiles as spread; not part of "all"), on the velocity
of a fused TGV run three steps old: (a) x3d_particles_advance (HIP events) for 2^16, 2^20 and 2^22 particles, orders 2 and 4,
tracers and inertial, straight after seed_uniform (random order) and straight after a sort, in particles per second and in the
field bytes the stencils ask for (order^3 x 3 values per particle); beside them the sort (keys + radix sort + gather: the first
one from random order as one sample, then the median on the sorted state) and x3d_probe_sample for 4096 probes; (b) the choice
of the default sort_every: 64 steps with 2^20 order-4 tracers at sort_every 0, 1, 8 and 64, HIP events around Particles.update
(advance and the sorts that fall due), mean per step; (c) 20 fused RK3 steps with nothing attached, with Probes at every step
(which gives up the more=True deferral as the particles do) and with 2^20 order-4 tracers (never sorted): wall time.  No gate; (d)
the launches of particles on several ranks, driven through the C ABI in this one process on a geometry that treats the box
as the lower of two z slabs with itself as both neighbours (its own messages are what it receives), 2^20 order-4 tracers:
ghost pack + unpack, move, emigrate + immigrate and sample, with the fused x3d_particles_advance timed in the same loop;
gate t_move + t_sample <= 1.25 t_advance (the split reads and writes the twelve state rows once more: 192 B per particle
against the 1536 B its stencils fetch, doubled for margin).  --particles-part mp runs (d) alone.  The lines are appended to
profiles/particles.jsonl.

--family scalars (csrc/scalars.hip, x3d2_amd/scalars.py), at --snap-n (512) cubed, HIP events, the two sides of a comparison
timed in turn inside one loop: (a) x3d_scalars_couple at ns = 1, up = y next to x3d_vecadd on the same blocks (both move three
streams); gate t_couple <= 1.15 t_vecadd; (b) x3d_scalars_couple at ns = 3 with an oblique up and G != 0 next to the twelve
x3d_vecadd calls that compose the same terms; (c) x3d_scalars_profile_sums at ns = 1 next to x3d_stats_profile_sums; (d) 20
fused RK3 TGV steps with one passive species against the same run with ri = 1: what giving up the deferred branch costs (wall
time).  The lines are appended to profiles/scalars.jsonl.

--family forcing (csrc/forcing.hip, x3d2_amd/forcing.py), at --snap-n (512) cubed on the velocity of make_hit, HIP events, the two
sides of a comparison timed in turn inside one loop, median of --stat-iters with the quartiles: x3d_forcing_project next to
x3d_stats_profile_sums on the same fields (both read u, v, w once) and x3d_forcing_synth next to three x3d_vecadd calls on the
same blocks (x = y: the same bytes), at the default band (k_hi = 2.5: M = 2; gates 1.25 x) and at k_hi = 4.5 (M = 4: reported only); Forcing.add as a
whole; 20 fused RK3 steps of make_hit without and with the forcing (wall time, no gate).  The lines are appended to
profiles/forcing.jsonl.

--family feedback (csrc/particles.hip x3d_particles_feedback_*, x3d2_amd/particles.py Feedback), at --snap-n (512) cubed with 2^20
inertial particles from seed_uniform on the velocity of make_hit, HIP events, the two sides of a comparison timed in turn inside
one loop, median of --stat-iters with the quartiles: Feedback.add (the eight passes) next to three x3d_vecadd calls on the same
blocks (x = y; what a dense force field would cost per sub-step at the least: the gate, no margin); the record build (keys, two
sorts, records) next to Particles.sort and x3d_particles_advance; the record build at 2^22 particles; 20 fused RK3 steps of
make_hit with the particles one-way and two-way (wall time, no gate).  The lines are appended to profiles/feedback.jsonl.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def bench_stats(args):
    """one JSON line per (op, n) of the "statistics sample" family"""
    import ctypes

    import torch
    from x3d2_amd import Mesh, _lib
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.common import DIR_X, VERT
    per = ("periodic",) * 2
    rb = 4 if _lib.SINGLE else 8
    for n in (256, 512):
        mesh = Mesh((n, n, n), (1, 1, 1), (6.283185307179586,) * 3, per, per, per)
        b = HipBackend(mesh)
        al = b.allocator
        u, v, w, tmp = (al.get_block(DIR_X, VERT) for _ in range(4))
        means = [al.get_block(DIR_X, VERT) for _ in range(9)]
        rng = np.random.default_rng(0)
        for f in (u, v, w):
            b.set_field_data(f, rng.standard_normal((n, n, n), dtype=np.float32))
        for f in means:
            f.fill(0.0)
        prof, sums = (torch.zeros(9 * n, dtype=_lib.torch_real(), device=b.device) for _ in range(2))
        dof, inc = n ** 3, 0.125

        def composed():
            for x, m in zip((u, v, w), means[:3]):
                b.vecadd(inc, x, 1.0 - inc, m)
            for (x, y), m in zip(((u, u), (v, v), (w, w), (u, v), (u, w), (v, w)), means[3:]):
                b.veccopy(tmp, x)
                b.vecmult(tmp, y)
                b.vecadd(inc, tmp, 1.0 - inc, m)

        def profile():
            b.stats_profile_sums(u, v, w, 2, sums)
            b.stats_profile_accumulate(prof, sums, 1.0 / (n * n), inc)

        cases = (("statistics sample: fused 3-D update", lambda: b.stats_update_uvw(u, v, w, means, inc), 21),
                 ("statistics sample: composed from veccopy/vecmult/vecadd", composed, 57),
                 ("statistics sample: profile update (dir_keep = y)", profile, 3),
                 ("scalar_product (k_reduce) on the same field", lambda: b.scalar_product(u, v), 2))
        ms_of = {}
        for name, fn, reals in cases:
            ms = ctypes.c_float()
            times = []
            for i in range(args.stat_warmup + args.stat_iters):
                _lib.check(b.lib.x3d_timer_start(b.h))
                fn()
                _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
                if i >= args.stat_warmup:
                    times.append(ms.value)
            t = float(np.median(times))
            ms_of[name] = t
            gbs = reals * rb * dof / t / 1e6
            row = {"op": name, "n": n, "real_bytes": rb, "ms_median": t, "ms_min": float(min(times)), "launches": len(times),
                   "bytes_per_dof": reals * rb, "GBs": gbs, "ceiling": gbs / 6200.0}
            if name.endswith("fused 3-D update"):
                fused = t
            if "composed" in name:
                row["fused_over_composed"] = fused / t
            print(json.dumps(row))
        del b, al, u, v, w, tmp, means
        torch.cuda.empty_cache()


def bench_ibm(args):
    """one JSON line per measurement of the "ibm" family"""
    import ctypes
    from types import SimpleNamespace

    import torch
    from x3d2_amd import Mesh, _lib, make_cylinder
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.common import DIR_X, VERT, X_FACE
    from x3d2_amd.ibm import Ibm, cylinder_mask
    per = ("periodic",) * 2
    n, twopi, step_ms = 512, 6.283185307179586, 40.0
    mesh = Mesh((n, n, n), (1, 1, 1), (twopi,) * 3, per, per, per)
    b = HipBackend(mesh)
    al = b.allocator
    u, v, w, iu, iv, iw, mask = (al.get_block(DIR_X, VERT) for _ in range(7))
    rng = np.random.default_rng(0)
    for f in (u, v, w):
        b.set_field_data(f, 1.0 + 0.1 * rng.standard_normal((n, n, n), dtype=np.float32))
    for f, c in ((iu, 1.0), (iv, 0.0), (iw, 0.0)):
        f.fill(c)
    ep1 = cylinder_mask(mesh, (twopi / 4, twopi / 2), twopi / 40)
    mask.fill(1.0)
    b.set_field_data(mask, ep1)
    ibm = Ibm(SimpleNamespace(backend=b), ep1)
    dx, gdt = twopi / n, 1e-3
    rb = 4 if _lib.SINGLE else 8

    def three_vecmult():
        for f in (u, v, w):
            b.vecmult(f, mask)

    def new_path():
        p = b.outflow_params(u, gdt, dx)
        b.cylinder_apply_bc(u, v, w, iu, iv, iw, p)
        ibm.body(u, v, w)

    def composed_path():
        uxmax, _ = b.slice_max_sum(u, n - 1)
        _, s_in = b.slice_max_sum(u, 1)
        _, s_out = b.slice_max_sum(u, n)
        out_vel, frd = uxmax * gdt / dx, s_in / (n * n) - s_out / (n * n)
        for f, st in ((u, iu), (v, iv), (w, iw)):
            b.field_set_face_from_field(f, st, out_vel, X_FACE, flow_rate_diff=frd)
        three_vecmult()

    def timed(fn):
        ms, times, walls = ctypes.c_float(), [], []
        s0 = b.sync_count()
        for i in range(args.stat_warmup + args.stat_iters):
            b.sync()
            t0 = time.perf_counter()
            _lib.check(b.lib.x3d_timer_start(b.h))
            fn()
            _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
            if i >= args.stat_warmup:
                times.append(ms.value)
                walls.append((time.perf_counter() - t0) * 1e3)
        syncs = (b.sync_count() - s0) / float(args.stat_warmup + args.stat_iters)
        return float(np.median(times)), float(min(times)), float(np.median(walls)), syncs

    res = {}
    for name, fn in (("ibm.body (work list)", lambda: ibm.body(u, v, w)), ("one vecmult by a device mask", lambda: b.vecmult(u, mask)),
                     ("three vecmult by a device mask", three_vecmult),
                     ("boundary path: outflow_params + cylinder_apply_bc + ibm.body", new_path),
                     ("boundary path composed: 3 slice_max_sum + 3 set_face_from_field + 3 vecmult", composed_path)):
        t, tmin, wall, syncs = timed(fn)
        res[name] = t
        row = {"family": "ibm", "op": name, "n": n, "real_bytes": rb, "ms_median": t, "ms_min": tmin, "wall_ms_median": wall,
               "launch_groups": args.stat_iters, "stream_syncs_per_call": syncs, "step_share": t / step_ms}
        if name.startswith("ibm.body"):
            row.update(n_segments=ibm.n_segments, n_masked=ibm.n_masked, masked_fraction=ibm.n_masked / float(n ** 3),
                       bytes_moved=ibm.n_segments * 64 * rb * 7, bytes_of_one_vecmult=3 * rb * n ** 3)
        if name.startswith("three"):
            row["body_over_one_vecmult"] = res["ibm.body (work list)"] / res["one vecmult by a device mask"]
            row["body_over_three_vecmult"] = res["ibm.body (work list)"] / t
        if "composed" in name:
            row["new_over_composed"] = res["boundary path: outflow_params + cylinder_apply_bc + ibm.body"] / t
        print(json.dumps(row), flush=True)
    del ibm, b, al, u, v, w, iu, iv, iw, mask
    torch.cuda.empty_cache()
    # the whole case, both forms from the same process, in this order
    for dense in (False, True):
        if dense:
            os.environ["X3D_NO_IBM_SPARSE"] = "1"
        else:
            os.environ.pop("X3D_NO_IBM_SPARSE", None)
        case = make_cylinder((257, 128, 32), fused=True)
        sb = case.solver.backend
        for it in range(1, 4):
            case.step(it)
        sb.sync()
        t0 = time.perf_counter()
        for it in range(4, 24):
            case.step(it)
        sb.sync()
        t = (time.perf_counter() - t0) / 20 * 1e3
        row = case.postprocess(23, 23 * case.solver.dt)
        print(json.dumps({"family": "ibm", "op": "make_cylinder((257,128,32)), fused, AB3: 20 steps", "dense_mask": dense,
                          "ms_per_step": t, "n_segments": case.solver.ibm.n_segments, "n_masked": case.solver.ibm.n_masked,
                          "enstrophy": row[1], "div_u_max": row[2], "out_vel": case.out_vel}), flush=True)
        del case, sb
        torch.cuda.empty_cache()
    os.environ.pop("X3D_NO_IBM_SPARSE", None)


def bench_snapshot(args):
    """one JSON line per measurement of the "snapshot" family"""
    import ctypes
    import tempfile

    import torch
    from x3d2_amd import _lib, make_tgv
    from x3d2_amd.common import DIR_X, DIR_Y, DIR_Z, VERT
    from x3d2_amd.snapshot import SnapshotConfig, Snapshots
    n, rb = args.snap_n, 4 if _lib.SINGLE else 8
    fields = ("pressure", "vorticity", "qcriterion")
    tmp = tempfile.mkdtemp(prefix="x3d_snap_")
    case = make_tgv(n, fused=True)
    s = case.solver
    b, al = s.backend, s.backend.allocator
    s.keep_pressure = True
    case.step(1, want_pressure=True)
    s.flush_grad()
    nxp = b.padded_dims[0]

    # (a) the pack kernel alone
    g = s.velocity_gradients()
    pv = al.get_block(DIR_X, VERT)
    b.tds_apply(pv, s.pressure, s.zdirps.interpl_p2v, DIR_Z)
    variables = [("copy", s.u, 1.0), ("copy", s.v, 1.0), ("copy", s.w, 1.0), ("copy", pv, 1.0 / s.dt), ("vort", g), ("qcrit", g)]
    for stride in ((1, 1, 1), (2, 2, 2)):
        cnt = tuple((n + st - 1) // st for st in stride)
        for dt in (np.float32, np.float64):
            size = np.dtype(dt).itemsize
            out = torch.empty(6 * cnt[0] * cnt[1] * cnt[2] * size, dtype=torch.uint8, device=b.device)
            ms, times = ctypes.c_float(), []
            for i in range(args.stat_warmup + args.stat_iters):
                _lib.check(b.lib.x3d_timer_start(b.h))
                b.snapshot_pack(variables, (0, 0, 0), stride, cnt, out, dt)
                _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
                if i >= args.stat_warmup:
                    times.append(ms.value)
            t = float(np.median(times))
            row_bytes = n * rb if stride[0] * rb < 128 else cnt[0] * 128  # (kept rows only; every line of a kept row)
            src = (4 + 18) * cnt[1] * cnt[2] * row_bytes  # four COPY sources, nine gradient blocks read by each of vort, qcrit
            total = src + out.numel()
            print(json.dumps({"family": "snapshot", "op": "pack, six variables", "n": n, "stride": stride, "out_bytes": size,
                              "real_bytes": rb, "ms_median": t, "ms_min": float(min(times)), "launches": len(times),
                              "source_bytes": src, "output_bytes": out.numel(), "GBs": total / t / 1e6,
                              "ceiling": total / t / 1e6 / 6200.0, "row_pitch": nxp}), flush=True)
            del out
    for f in g + [pv]:
        al.release_block(f)

    # (b) host-visible cost of Snapshots.write against the composed path
    stride = (2, 2, 2)
    snap = Snapshots(s, SnapshotConfig(snapshot_freq=1, snapshot_prefix=os.path.join(tmp, "b"), output_stride=stride,
                                       snapshot_sp=True, output_fields=fields))

    def composed():
        gg = s.velocity_gradients()
        o = al.get_block(DIR_X, VERT)
        res = []
        for fn in (b.compute_vorticity, b.compute_qcriterion):
            fn(o, *gg)
            o.set_data_loc(VERT)
            res.append(b.get_field_data(o)[::2, ::2, ::2].astype(np.float32))
        for f in (s.u, s.v, s.w):
            res.append(b.get_field_data(f)[::2, ::2, ::2].astype(np.float32))
        t1, t2 = al.get_block(DIR_X, VERT), al.get_block(DIR_X, VERT)
        b.tds_apply(t1, s.pressure, s.zdirps.interpl_p2v, DIR_Z)
        b.tds_apply(t2, t1, s.ydirps.interpl_p2v, DIR_Y)
        b.tds_apply(t1, t2, s.xdirps.interpl_p2v, DIR_X)
        t1.set_data_loc(VERT)
        res.append((b.get_field_data(t1) * (1.0 / s.dt))[::2, ::2, ::2].astype(np.float32))
        for f in gg + [o, t1, t2]:
            al.release_block(f)
        return res

    for name, fn, after in (("Snapshots.write, call to return", lambda it: snap.write(it), snap.finalise),
                            ("composed: 6 get_field_data + 2 compute_* + numpy stride / astype", lambda it: composed(), None)):
        walls, s0 = [], b.sync_count()
        for i in range(3 + 10):
            b.sync()
            t0 = time.perf_counter()
            fn(i + 1)
            w = (time.perf_counter() - t0) * 1e3
            if after is not None:
                after()  # (outside the timed region: the files are written, both buffers are free again)
            if i >= 3:
                walls.append(w)
        print(json.dumps({"family": "snapshot", "op": name, "n": n, "stride": stride, "out_bytes": 4,
                          "wall_ms_median": float(np.median(walls)), "wall_ms_q1": float(np.percentile(walls, 25)),
                          "wall_ms_q3": float(np.percentile(walls, 75)), "wall_ms_min": float(min(walls)), "calls": len(walls),
                          "stream_syncs": b.sync_count() - s0}), flush=True)
    del snap, case, s, b, al
    torch.cuda.empty_cache()

    # (c) a 20-step run with and without snapshots
    res = {}
    for with_snap in (False, True):
        case = make_tgv(n, fused=True)
        if with_snap:
            case.snapshots = Snapshots(case.solver, SnapshotConfig(snapshot_freq=5, snapshot_prefix=os.path.join(tmp, "c"),
                                                                   output_stride=stride, snapshot_sp=True, output_fields=fields))
        case.run(n_iters=3)
        case.solver.backend.sync()
        t0 = time.perf_counter()
        case.run(n_iters=23)
        case.solver.backend.sync()
        res[with_snap] = (time.perf_counter() - t0) * 1e3
        del case
        torch.cuda.empty_cache()
    print(json.dumps({"family": "snapshot", "op": "TGV, fused, RK3: 20 steps, snapshot_freq 5", "n": n, "stride": stride,
                      "out_bytes": 4, "wall_ms_without": res[False], "wall_ms_with": res[True], "snapshots": 4,
                      "added_ms_per_snapshot": (res[True] - res[False]) / 4.0}), flush=True)


def bench_checkpoint(args):
    """one JSON line per measurement of the "checkpoint" family"""
    import ctypes
    import tempfile

    import torch
    from x3d2_amd import _lib, make_tgv
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints
    from x3d2_amd.common import DIR_X, VERT
    n, rb = args.snap_n, 4 if _lib.SINGLE else 8
    tmp = tempfile.mkdtemp(prefix="x3d_ckpt_")
    case = make_tgv(n, fused=True, time_intg="AB4")
    s = case.solver
    b, al = s.backend, s.backend.allocator
    case.step(1)
    s.flush_grad()
    dims = tuple(int(v) for v in s.mesh.get_dims(VERT))
    npts = int(np.prod(dims))
    state = [s.u, s.v, s.w] + [f for row in s.time_integrator.olds for f in row]  # 12 blocks

    # (a) the pack launch alone, 3 and 12 blocks
    for nblock in (3, 12):
        _, _, total = b.checkpoint_layout(nblock, npts)
        buf = torch.empty(total, dtype=torch.uint8, device=b.device)
        ms, times = ctypes.c_float(), []
        for i in range(args.stat_warmup + args.stat_iters):
            _lib.check(b.lib.x3d_timer_start(b.h))
            b.checkpoint_pack(state[:nblock], dims, buf)
            _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
            if i >= args.stat_warmup:
                times.append(ms.value)
        t = float(np.median(times))
        moved = 2 * nblock * npts * rb  # every interior element read once and written once
        print(json.dumps({"family": "checkpoint", "op": "pack with checksums", "n": n, "blocks": nblock, "real_bytes": rb,
                          "ms_median": t, "ms_min": float(min(times)), "launches": len(times), "bytes": moved,
                          "GBs": moved / t / 1e6, "ceiling": moved / t / 1e6 / 6200.0, "row_pitch": b.padded_dims[0]}),
              flush=True)
        del buf
    torch.cuda.empty_cache()

    # (b) host-visible cost of Checkpoints.write against the only route there was: get_field_data of the same blocks
    ck = Checkpoints(s, CheckpointConfig(checkpoint_freq=1, checkpoint_prefix=os.path.join(tmp, "b")), case)
    ck.ring.on_land = lambda payload, raw: None  # (the copies are waited for, no file is written here)
    for name, fn, after in (("Checkpoints.write, call to return", lambda it: ck.write(it), ck.ring.drain),
                            ("composed: 12 get_field_data", lambda it: [b.get_field_data(f, VERT) for f in state], None)):
        walls, s0 = [], b.sync_count()
        for i in range(2 + 5):
            b.sync()
            t0 = time.perf_counter()
            fn(i + 1)
            w = (time.perf_counter() - t0) * 1e3
            if after is not None:
                after()  # (outside the timed region: the copy has landed)
            if i >= 2:
                walls.append(w)
        print(json.dumps({"family": "checkpoint", "op": name, "n": n, "blocks": 12, "wall_ms_median": float(np.median(walls)),
                          "wall_ms_q1": float(np.percentile(walls, 25)), "wall_ms_q3": float(np.percentile(walls, 75)),
                          "wall_ms_min": float(min(walls)), "calls": len(walls), "stream_syncs": b.sync_count() - s0}), flush=True)
    del ck, case, s, b, al, state
    torch.cuda.empty_cache()

    # (c) a 20-step run with and without checkpoints; poll() writes the file on the host thread (np.savez)
    res, in_poll = {}, 0.0
    for with_ckpt in (False, True):
        case = make_tgv(n, fused=True)
        if with_ckpt:
            ck = Checkpoints(case.solver, CheckpointConfig(checkpoint_freq=5, checkpoint_prefix=os.path.join(tmp, "c"),
                                                           keep_checkpoint=False), case)
            inner = ck.ring.on_land

            def timed_write(payload, raw):
                nonlocal in_poll
                t1 = time.perf_counter()
                out = inner(payload, raw)
                in_poll += (time.perf_counter() - t1) * 1e3
                return out

            ck.ring.on_land = timed_write
            case.checkpoints = ck
        case.run(n_iters=3)
        case.solver.backend.sync()
        in_poll = 0.0
        t0 = time.perf_counter()
        case.run(n_iters=23)
        case.solver.backend.sync()
        res[with_ckpt] = (time.perf_counter() - t0) * 1e3
        del case
        torch.cuda.empty_cache()
    print(json.dumps({"family": "checkpoint", "op": "TGV, fused, RK3: 20 steps, checkpoint_freq 5", "n": n,
                      "wall_ms_without": res[False], "wall_ms_with": res[True], "checkpoints": 4,
                      "added_ms_per_checkpoint": (res[True] - res[False]) / 4.0, "ms_in_file_writes": in_poll}), flush=True)


def bench_spectra(args):
    """one JSON line per case of the "spectra" family"""
    import ctypes

    import torch
    from x3d2_amd import _lib, make_channel, make_tgv
    from x3d2_amd.spectra import Spectra, SpectraConfig
    rb = 4 if _lib.SINGLE else 8

    def timed(b, fn):
        ms, times = ctypes.c_float(), []
        for i in range(args.stat_warmup + args.stat_iters):
            _lib.check(b.lib.x3d_timer_start(b.h))
            fn()
            _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
            if i >= args.stat_warmup:
                times.append(ms.value)
        return float(np.median(times)), float(min(times)), len(times)

    def row(op, dims, t, tmin, n, nbytes=None, **more):
        out = {"op": op, "dims": list(dims), "real_bytes": rb, "ms_median": t, "ms_min": tmin, "launches": n,
               "step_share": t / 40.0}
        if nbytes is not None:
            out.update(bytes=nbytes, GBs=nbytes / t / 1e6, ceiling=nbytes / t / 1e6 / 6200.0)
        out.update(more)
        print(json.dumps(out), flush=True)

    n = args.snap_n
    case = make_tgv(n, fused=True)
    s = case.solver
    b = s.backend
    sp = Spectra(s, SpectraConfig(mode="shell", initspec=1))
    pf = b.poisson_fft
    nxs = (n // 2 + 1 + 7) // 8 * 8
    spec_bytes = n * n * nxs * 2 * rb
    sp.sample()
    t, tmin, k = timed(b, lambda: _lib.check(b.lib.x3d_spectra_reduce(sp.h, pf.h, 0)))
    row("spectra: shell binning alone (one field)", (n, n, n), t, tmin, k, spec_bytes, nbins=sp.layout.nbins,
        workgroups=sp.groups)
    t, tmin, k = timed(b, lambda: b.scalar_product(s.u, s.v))
    row("scalar_product (k_reduce) on the same box", (n, n, n), t, tmin, k, 2 * rb * n ** 3)
    t, tmin, k = timed(b, sample_of(sp))
    row("spectra: three-field shell sample (3 transforms + 3 binnings + mean)", (n, n, n), t, tmin, k)

    # the composed path: the spectrum to the host, binned there (what the device reduction replaces)
    m = np.arange(n)
    k1 = np.where(m <= n // 2, m, m - n).astype(np.float64) ** 2
    wx = np.full(n // 2 + 1, 2.0)
    wx[0] = 1.0
    if n % 2 == 0:
        wx[n // 2] = 1.0
    bins = np.floor(np.sqrt((k1[None, None, :n // 2 + 1] + k1[None, :, None]) + k1[:, None, None]) / sp.layout.dk
                    + 0.5).astype(np.int64).reshape(-1)
    times = []
    for _ in range(2):  # (seconds each: the host bins 3 x 67 million modes)
        b.sync()
        t0 = time.perf_counter()
        for f in (s.u, s.v, s.w):
            pf.fft_forward(f)
            c = pf.get_spectral()
            e = (0.5 * wx)[None, None, :] * (c.real * c.real + c.imag * c.imag) / float(n) ** 6
            np.bincount(bins, weights=e.reshape(-1), minlength=sp.layout.nbins)
        times.append((time.perf_counter() - t0) * 1e3)
    row("spectra: composed, get_spectral + numpy binning, three fields (wall clock)", (n, n, n), float(np.median(times)),
        float(min(times)), len(times))
    del case, s, sp, pf, b, bins
    torch.cuda.empty_cache()
    # plane mode at the channel's production size
    dims = (1024, 257, 512)
    case = make_channel(dims, L=(8.0, 2.0, 4.0), fused=True)
    s = case.solver
    b = s.backend
    sp = Spectra(s, SpectraConfig(mode="plane", initspec=1))
    sp.sample()
    pnxs = (dims[0] // 2 + 1 + 7) // 8 * 8
    t, tmin, k = timed(b, lambda: _lib.check(b.lib.x3d_spectra_reduce(sp.h, None, 0)))
    row("spectra: plane reduction alone (one field)", dims, t, tmin, k, dims[2] * dims[1] * pnxs * 2 * rb, workgroups=sp.groups)
    t, tmin, k = timed(b, sample_of(sp))
    row("spectra: three-field plane sample (3 2-D transforms + 3 reductions + mean)", dims, t, tmin, k)


def spread(times):
    q1, med, q3 = (float(v) for v in np.percentile(times, [25, 50, 75]))
    return {"ms_median": med, "ms_q1": q1, "ms_q3": q3, "ms_min": float(min(times)), "samples": len(times)}


def timed_events(args, b, fn):
    """HIP-event ms of fn() on the backend's stream: --stat-iters samples after --stat-warmup"""
    import ctypes
    from x3d2_amd import _lib
    ms, times = ctypes.c_float(), []
    for i in range(args.stat_warmup + args.stat_iters):
        _lib.check(b.lib.x3d_timer_start(b.h))
        fn()
        _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
        if i >= args.stat_warmup:
            times.append(ms.value)
    return times


def timed_wall(args, b, fn):
    """wall-clock ms of fn() between two device syncs"""
    times = []
    for i in range(args.stat_warmup + args.stat_iters):
        b.sync()
        t0 = time.perf_counter()
        fn()
        b.sync()
        if i >= args.stat_warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return times


def bench_diagnostics(args):
    """one JSON line per measurement of the "diagnostics" family, printed and appended to profiles/diagnostics.jsonl"""
    import tempfile

    import torch
    from x3d2_amd import _lib, make_tgv
    from x3d2_amd.diagnostics import Diagnostics, DiagnosticsConfig
    n, rb = args.snap_n, 4 if _lib.SINGLE else 8
    tmp = tempfile.mkdtemp(prefix="x3d_diag_")
    out_path = os.path.join(ROOT, "profiles", "diagnostics.jsonl")

    def emit(row):
        row = dict({"family": "diagnostics", "n": n, "real_bytes": rb}, **row)
        line = json.dumps(row)
        print(line, flush=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")

    events, wall = (lambda b, fn: timed_events(args, b, fn)), (lambda b, fn: timed_wall(args, b, fn))
    case = make_tgv(n, fused=True)
    s = case.solver
    b, al = s.backend, s.backend.allocator
    case.step(1)
    s.flush_grad()
    dg = Diagnostics(s, DiagnosticsConfig(prefix=os.path.join(tmp, "a")))
    # (a) the reduction launches alone, on gradients computed once
    grads = s.velocity_gradients()
    t = spread(events(b, lambda: dg.reduce(s.u, s.v, s.w, grads)))
    nbytes = 12 * rb * n ** 3
    emit(dict({"op": "x3d_diag_reduce: both launches (12 blocks read)", "bytes": nbytes, "GBs": nbytes / t["ms_median"] / 1e6,
               "ceiling": nbytes / t["ms_median"] / 1e6 / 6200.0, "row_pitch": b.padded_dims[0]}, **t))
    t = spread(events(b, lambda: b.scalar_product(s.u, s.v)))
    nbytes = 2 * rb * n ** 3
    emit(dict({"op": "x3d_scalar_product (k_reduce) on the same box", "bytes": nbytes, "GBs": nbytes / t["ms_median"] / 1e6,
               "ceiling": nbytes / t["ms_median"] / 1e6 / 6200.0}, **t))
    for g in grads:
        al.release_block(g)
    # (b) a whole sample, (c) the monitoring row it replaces: wall clock around a device sync, same state, same process
    count = [0]

    def sample():
        count[0] += 1
        dg.sample(count[0])
        dg.poll()

    s0 = b.sync_count()
    t = spread(wall(b, sample))
    emit(dict({"op": "Diagnostics sample: 9 gradients + reduction + divergence + max / sum (wall clock)",
               "stream_syncs_per_call": (b.sync_count() - s0) / float(args.stat_warmup + args.stat_iters)}, **t))
    dg.finalise()

    def monitoring():
        case.monitoring.write_step(0.0, s.u, s.v, s.w)
        case.monitoring.kinetic_energy()

    s0 = b.sync_count()
    t2 = spread(wall(b, monitoring))
    emit(dict({"op": "Monitoring.write_step + kinetic_energy (wall clock)",
               "stream_syncs_per_call": (b.sync_count() - s0) / float(args.stat_warmup + args.stat_iters)}, **t2))
    emit({"op": "gate: sample faster than monitoring", "sample_ms_median": t["ms_median"], "monitoring_ms_median": t2["ms_median"],
          "passed": bool(t["ms_median"] < t2["ms_median"])})
    del case, s, b, al, dg, grads
    torch.cuda.empty_cache()
    # (d) a 20-step run with a row per step against the same run without
    res = {}
    for with_diag in (False, True):
        case = make_tgv(n, fused=True)
        if with_diag:
            case.diagnostics = Diagnostics(case.solver, DiagnosticsConfig(prefix=os.path.join(tmp, "d")))
        case.run(n_iters=3)
        case.solver.backend.sync()
        t0 = time.perf_counter()
        case.run(n_iters=23)
        case.solver.backend.sync()
        res[with_diag] = (time.perf_counter() - t0) * 1e3
        del case
        torch.cuda.empty_cache()
    emit({"op": "TGV, fused, RK3: 20 steps, idiagfreq 1", "wall_ms_without": res[False], "wall_ms_with": res[True],
          "added_ms_per_step": (res[True] - res[False]) / 20.0})


def bench_budgets(args):
    """one JSON line per measurement of the "budgets" family, printed and appended to profiles/budgets.jsonl"""
    import torch
    from x3d2_amd import _lib, make_tgv
    from x3d2_amd.budgets import Budgets, BudgetsConfig
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.diagnostics import Diagnostics, DiagnosticsConfig
    import tempfile
    n, rb = args.snap_n, 4 if _lib.SINGLE else 8
    tmp = tempfile.mkdtemp(prefix="x3d_bud_")
    out_path = os.path.join(ROOT, "profiles", "budgets.jsonl")

    def emit(row):
        row = dict({"family": "budgets", "n": n, "real_bytes": rb}, **row)
        line = json.dumps(row)
        print(line, flush=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")

    events, wall = (lambda b, fn: timed_events(args, b, fn)), (lambda b, fn: timed_wall(args, b, fn))
    case = make_tgv(n, fused=True)
    s = case.solver
    b, al = s.backend, s.backend.allocator
    case.step(1)
    s.flush_grad()
    bud = Budgets(s, BudgetsConfig(initbud=1, profile_dir=2, pressure=False, prefix=os.path.join(tmp, "b")))
    dg = Diagnostics(s, DiagnosticsConfig(prefix=os.path.join(tmp, "a")))
    # (a) the sums launches alone, on gradients computed once and a thirteenth block in the pressure's place, next to
    # x3d_diag_reduce in the same process: both are read-only streams
    grads = s.velocity_gradients()
    p = al.get_block(DIR_X, VERT)
    b.veccopy(p, s.u)
    tb = spread(events(b, lambda: b.budget_profile_sums(s.u, s.v, s.w, p, grads, 2, 1.0 / s.dt, bud.sums)))
    nbytes = 13 * rb * n ** 3
    emit(dict({"op": "x3d_budget_profile_sums: both launches (13 blocks read)", "bytes": nbytes,
               "GBs": nbytes / tb["ms_median"] / 1e6, "ceiling": nbytes / tb["ms_median"] / 1e6 / 6200.0,
               "row_pitch": b.padded_dims[0]}, **tb))
    td = spread(events(b, lambda: dg.reduce(s.u, s.v, s.w, grads)))
    nbytes = 12 * rb * n ** 3
    emit(dict({"op": "x3d_diag_reduce: both launches (12 blocks read)", "bytes": nbytes, "GBs": nbytes / td["ms_median"] / 1e6,
               "ceiling": nbytes / td["ms_median"] / 1e6 / 6200.0}, **td))
    limit = 1.25 * (104.0 / 96.0) * td["ms_median"]
    emit({"op": "gate: t_budget <= 1.25 (104 / 96) t_diag_reduce", "budget_ms_median": tb["ms_median"],
          "diag_reduce_ms_median": td["ms_median"], "ratio": tb["ms_median"] / td["ms_median"], "limit_ms": limit,
          "passed": bool(tb["ms_median"] <= limit)})
    al.release_block(p)
    for g in grads:
        al.release_block(g)
    # (b) a whole update (no pressure: a TGV run keeps none), (c) the composed host path it replaces: thirteen
    # get_field_data plus numpy moments; wall clock around a device sync, same state, same process
    tu = spread(wall(b, sample_of(bud)))
    emit(dict({"op": "Budgets.update, pressure=False: 9 gradients + sums + recurrence (wall clock)"}, **tu))

    def host_path():
        taken = s.velocity_gradients() + [al.get_block(DIR_X, VERT)]
        a = [b.get_field_data(f) for f in [s.u, s.v, s.w] + taken]
        for f in taken:
            al.release_block(f)
        vel, pp, g = a[:3], a[12], [a[3:6], a[6:9], a[9:12]]
        pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
        mean = lambda x: x.mean(axis=(0, 2))
        out = [mean(x) for x in vel] + [mean(pp)] + [mean(pp * pp)] + [mean(pp * x) for x in vel]
        for i, j in pairs:
            uu = vel[i] * vel[j]
            out += [mean(uu), mean(uu * vel[1]), mean(g[i][0] * g[j][0] + g[i][1] * g[j][1] + g[i][2] * g[j][2]),
                    mean(pp * (g[i][j] + g[j][i]))]
        out += [mean(x) for row in g for x in row]
        return out

    saved = args.stat_warmup, args.stat_iters
    args.stat_warmup, args.stat_iters = 0, 3  # (seconds per call)
    th = spread(wall(b, host_path))
    args.stat_warmup, args.stat_iters = saved
    emit(dict({"op": "composed host path: 13 get_field_data + numpy moments (wall clock)"}, **th))
    emit({"op": "gate: update faster than the composed host path", "update_ms_median": tu["ms_median"],
          "host_ms_median": th["ms_median"], "passed": bool(tu["ms_median"] < th["ms_median"])})
    del case, s, b, al, bud, dg, grads, p
    torch.cuda.empty_cache()
    # (d) a 20-step run with a sample per step against the same run without
    res = {}
    for with_bud in (False, True):
        case = make_tgv(n, fused=True)
        if with_bud:
            case.budgets = Budgets(case.solver, BudgetsConfig(initbud=1, ibudfreq=1, pressure=False,
                                                              prefix=os.path.join(tmp, "d")))
        case.run(n_iters=3)
        case.solver.backend.sync()
        t0 = time.perf_counter()
        case.run(n_iters=23)
        case.solver.backend.sync()
        res[with_bud] = (time.perf_counter() - t0) * 1e3
        del case
        torch.cuda.empty_cache()
    emit({"op": "TGV, fused, RK3: 20 steps, ibudfreq 1, pressure=False", "wall_ms_without": res[False],
          "wall_ms_with": res[True], "added_ms_per_step": (res[True] - res[False]) / 20.0})


def sample_of(sp):
    count = [sp.sample_count]

    def sample():
        count[0] += 1
        sp.update(count[0])

    return sample


def bench_loads(args):
    """one JSON line per measurement of the "loads" family, printed and appended to profiles/loads.jsonl"""
    import ctypes
    import tempfile
    from types import SimpleNamespace

    import torch
    from x3d2_amd import Mesh, _lib, make_cylinder
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.ibm import Ibm, cylinder_mask
    from x3d2_amd.loads import Loads, LoadsConfig, weights
    from x3d2_amd.probes import Probes, ProbesConfig
    rb = 4 if _lib.SINGLE else 8
    tmp = tempfile.mkdtemp(prefix="x3d_loads_")
    out_path = os.path.join(ROOT, "profiles", "loads.jsonl")
    dims, L = (512, 256, 64), (20.0, 12.0, 6.0)

    def emit(row):
        row = dict({"family": "loads", "real_bytes": rb}, **row)
        line = json.dumps(row)
        print(line, flush=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")

    events = lambda b, fn: timed_events(args, b, fn)  # noqa: E731
    mesh = Mesh(dims, (1, 1, 1), L, ("dirichlet",) * 2, ("periodic",) * 2, ("periodic",) * 2)
    b = HipBackend(mesh)
    al = b.allocator
    u, v, w = (al.get_block(DIR_X, VERT) for _ in range(3))
    rng = np.random.default_rng(0)
    for f in (u, v, w):
        b.set_field_data(f, 1.0 + 0.1 * rng.standard_normal(dims[::-1], dtype=np.float32))
    ibm = Ibm(SimpleNamespace(backend=b), cylinder_mask(mesh, (L[0] / 4.0, L[1] / 2.0), 0.5))
    dp = ctypes.POINTER(ctypes.c_double)
    _lib.check(b.lib.x3d_ibm_set_weights(ibm.h, *[a.ctypes.data_as(dp) for a in weights(mesh)]))
    row_dev = torch.zeros(4, dtype=torch.float64, device=b.device)
    # (a) the body with and without the loads, alternating blocks of samples in one process
    tb = spread(events(b, lambda: ibm.body(u, v, w)))
    tl = spread(events(b, lambda: b.ibm_body_loads(ibm.h, u, v, w, row_dev.data_ptr(), 0)))
    tb2 = spread(events(b, lambda: ibm.body(u, v, w)))
    shape = {"dims": list(dims), "n_segments": ibm.n_segments, "n_masked": ibm.n_masked}
    emit(dict({"op": "x3d_ibm_body (work list)", "ms_median_repeat": tb2["ms_median"]}, **shape, **tb))
    emit(dict({"op": "x3d_ibm_body_loads: both launches", "above_body_ms": tl["ms_median"] - tb["ms_median"],
               "over_body": tl["ms_median"] / tb["ms_median"]}, **shape, **tl))
    # (b) 256 probes on a wake line and a cross line
    pts = np.stack([np.linspace(5.5, 19.5, 256), 6.0 + 2.0 * np.sin(np.arange(256.0)), np.linspace(0.1, 5.9, 256)], axis=1)
    stub = SimpleNamespace(backend=b, mesh=mesh, dt=0.0075, current_iter=0, u=u, v=v, w=w, flush_grad=lambda: None)
    pr = Probes(stub, ProbesConfig(pts, prefix=os.path.join(tmp, "p")))
    table = torch.zeros(3 * 256, dtype=torch.float64, device=b.device)
    tp = spread(events(b, lambda: b.probe_sample(pr.h, u, v, w, table.data_ptr())))
    emit(dict({"op": "x3d_probe_sample: 256 probes", "dims": list(dims)}, **tp))
    del ibm, pr, stub, b, al, u, v, w, row_dev, table
    torch.cuda.empty_cache()
    # (c), (d) the case: 20 timed steps, then 5 steps of a fresh run under the per-class timers for the launch groups
    cdims = (257, 128, 32)
    wake = np.stack([np.linspace(5.5, 19.5, 256), np.full(256, 6.0), np.full(256, 3.0)], axis=1)

    def attach(case, mode, tag):
        if mode in ("loads", "loads+probes"):
            case.loads = Loads(case.solver, LoadsConfig(prefix=os.path.join(tmp, tag + "_l")))
        if mode == "loads+probes":
            case.probes = Probes(case.solver, ProbesConfig(wake, prefix=os.path.join(tmp, tag + "_p")))

    res = {}
    for mode in ("none", "loads", "loads+probes"):
        case = make_cylinder(cdims, fused=True)
        sb = case.solver.backend
        attach(case, mode, "t")
        case.run(n_iters=3)  # (finalises what the three steps left: the timed run starts with empty tables)
        sb.sync()
        s0, t0 = sb.sync_count(), time.perf_counter()
        n_steps = 20
        # (run() opens with a postprocess row and closes with finalise(): the first waits the same way in every mode, the
        #  second waits for the landings of what the 20 steps left in the tables)
        case.run(n_iters=case.solver.current_iter + n_steps)
        sb.sync()
        wall = (time.perf_counter() - t0) * 1e3
        res[mode] = {"wall_ms": wall, "ms_per_step": wall / n_steps, "stream_syncs": sb.sync_count() - s0,
                     "ring_waits": sum(x.sync_count for x in (case.loads, case.probes) if x is not None),
                     "rows": 0 if case.loads is None else int(len(case.loads.rows()))}
        del case, sb
        torch.cuda.empty_cache()
        case = make_cylinder(cdims, fused=True)
        sb = case.solver.backend
        attach(case, mode, "c")
        case.step(1)
        sb.sync()
        sb.prof_enable(True)
        sb.prof_reset()
        case.solver.current_iter = 1
        for it in range(2, 7):
            case.step(it, more=(mode != "loads+probes"))
            case.solver.current_iter = it  # (as BaseCase.run does: Loads checks its count of body calls against it)
            if case.probes is not None:
                case.probes.update(it)
        sb.sync()
        groups = sum(sb.prof_get(k)[0] for k in sb.KINDS)
        sb.prof_enable(False)
        res[mode]["launch_groups_per_substep"] = groups / float(5 * case.solver.time_integrator.nstage)
        del case, sb
        torch.cuda.empty_cache()
    base = res["none"]
    for mode in ("none", "loads", "loads+probes"):
        r = res[mode]
        emit(dict({"op": "make_cylinder((257,128,32)), fused, AB3: 20 steps, " + mode, "dims": list(cdims),
                   "added_ms_per_step": r["ms_per_step"] - base["ms_per_step"],
                   "added_stream_syncs": r["stream_syncs"] - base["stream_syncs"],
                   "added_launch_groups_per_substep": r["launch_groups_per_substep"] - base["launch_groups_per_substep"]}, **r))
    # the landings finalise waits for: 20 rows at flush_every = 256 are one table per series
    emit({"op": "gate: host waits with Loads = those without + the landings finalise waits for",
          "added_stream_syncs": res["loads"]["stream_syncs"] - base["stream_syncs"], "landings_in_finalise": 1,
          "passed": bool(res["loads"]["stream_syncs"] - base["stream_syncs"] == 1 and res["loads"]["ring_waits"] == 0)})
    emit({"op": "gate: launches per sub-step grow by exactly one with Loads",
          "added_launch_groups_per_substep": res["loads"]["launch_groups_per_substep"] - base["launch_groups_per_substep"],
          "passed": bool(res["loads"]["launch_groups_per_substep"] - base["launch_groups_per_substep"] == 1.0)})


def bench_les(args):
    """one JSON line per measurement of the "les" family, printed and appended to profiles/les.jsonl"""
    import ctypes
    import tempfile

    import torch
    from x3d2_amd import _lib, make_tgv
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.diagnostics import Diagnostics, DiagnosticsConfig
    from x3d2_amd.les import Les, LesConfig
    n, rb = args.snap_n, 4 if _lib.SINGLE else 8
    tmp = tempfile.mkdtemp(prefix="x3d_les_")
    out_path = os.path.join(ROOT, "profiles", "les.jsonl")

    def emit(row):
        row = dict({"family": "les", "n": n, "real_bytes": rb}, **row)
        line = json.dumps(row)
        print(line, flush=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")

    case = make_tgv(n, fused=True)
    s = case.solver
    b, al = s.backend, s.backend.allocator
    case.step(1)
    s.flush_grad()
    # (a) the kernel alone; it overwrites its input, so the gradients are copied back (untimed) before every call
    grads = s.velocity_gradients()
    saved = [al.get_block(DIR_X, VERT) for _ in range(9)]
    for d, g in zip(saved, grads):
        b.veccopy(d, g)
    t_stress = {}
    for model in ("smagorinsky", "wale"):
        les = Les(s, LesConfig(model=model))
        ms, times = ctypes.c_float(), []
        for i in range(args.stat_warmup + args.stat_iters):
            for d, g in zip(saved, grads):
                b.veccopy(g, d)
            _lib.check(b.lib.x3d_timer_start(b.h))
            les.stress(grads)
            _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
            if i >= args.stat_warmup:
                times.append(ms.value)
        t = spread(times)
        t_stress[model] = t["ms_median"]
        nbytes = 16 * rb * n ** 3
        emit(dict({"op": "x3d_les_stress, %s: both launches (9 blocks read, 7 written)" % model, "bytes_per_dof": 16 * rb,
                   "TBs": nbytes / t["ms_median"] / 1e9, "ceiling": nbytes / t["ms_median"] / 1e6 / 6200.0,
                   "row_pitch": b.padded_dims[0], "monitor": les.monitor()}, **t))
    for g in grads:
        al.release_block(g)
    for f in saved:  # (the nine accumulators of the statistics update)
        f.fill(0.0)
    t = spread(timed_events(args, b, lambda: b.stats_update_uvw(s.u, s.v, s.w, saved, 0.125)))
    nbytes = 21 * rb * n ** 3
    emit(dict({"op": "x3d_stats_update_uvw on the same box (3 blocks read, 9 read and written)", "bytes_per_dof": 21 * rb,
               "TBs": nbytes / t["ms_median"] / 1e9, "ceiling": nbytes / t["ms_median"] / 1e6 / 6200.0}, **t))
    for f in saved:
        al.release_block(f)
    for model in ("smagorinsky", "wale"):
        limit = 1.25 * (128.0 / 168.0) * t["ms_median"]
        emit({"op": "gate: t_stress <= 1.25 (128 / 168) t_stats_update, %s" % model, "stress_ms_median": t_stress[model],
              "stats_update_ms_median": t["ms_median"], "limit_ms": limit, "passed": bool(t_stress[model] <= limit)})
    # (b) a whole Les.add next to a whole Diagnostics sample: wall clock around a device sync, same state, same process
    d = [al.get_block(DIR_X, VERT) for _ in range(3)]
    for f in d:
        f.fill(0.0)
    for model in ("smagorinsky", "wale"):
        les = Les(s, LesConfig(model=model))
        s0 = b.sync_count()
        t = spread(timed_wall(args, b, lambda: les.add(*d)))
        emit(dict({"op": "Les.add, %s: 9 gradients + stress + 9 accumulated derivatives (wall clock)" % model,
                   "stream_syncs_per_call": (b.sync_count() - s0) / float(args.stat_warmup + args.stat_iters)}, **t))
    for f in d:
        al.release_block(f)
    dg = Diagnostics(s, DiagnosticsConfig(prefix=os.path.join(tmp, "a")))
    count = [0]

    def sample():
        count[0] += 1
        dg.sample(count[0])
        dg.poll()

    t = spread(timed_wall(args, b, sample))
    emit(dict({"op": "Diagnostics sample: 9 gradients + reduction + divergence + max / sum (wall clock)"}, **t))
    dg.finalise()
    del case, s, b, al, dg, les, grads, saved, d
    torch.cuda.empty_cache()
    # (c) 20 steps with the model against the same run without (the parent's path)
    res = {}
    for model in (None, "smagorinsky", "wale"):
        case = make_tgv(n, fused=True)
        if model is not None:
            case.solver.les = Les(case.solver, LesConfig(model=model))
        case.run(n_iters=3)
        case.solver.backend.sync()
        t0 = time.perf_counter()
        case.run(n_iters=23)
        case.solver.backend.sync()
        res[model] = (time.perf_counter() - t0) * 1e3
        del case
        torch.cuda.empty_cache()
    for model in ("smagorinsky", "wale"):
        emit({"op": "TGV, fused, RK3: 20 steps, %s" % model, "wall_ms_without": res[None], "wall_ms_with": res[model],
              "ms_per_step_without": res[None] / 20.0, "added_ms_per_step": (res[model] - res[None]) / 20.0})
    # (d) the species' subgrid flux: x3d_les_scalar_flux for one and two species next to the fused statistics update in the
    # same loop; the kernel works in place, so the six gradients are copied back (untimed) before every timed call
    from x3d2_amd.common import DIR_Y, DIR_Z
    from x3d2_amd.les import NUT_BLOCK, PHI_BLOCK
    case = make_tgv(n, fused=True, n_species=1, pr_species=[0.7])
    s = case.solver
    b, al = s.backend, s.backend.allocator
    s.species[0].set_data_loc(VERT)
    b.veccopy(s.species[0], s.u)  # (a field with gradients: the case leaves its species unset)
    case.step(1)
    s.flush_grad()
    les = Les(s, LesConfig(model="wale", prt=0.85))
    grads = s.velocity_gradients()
    les.stress(grads)
    dirs = ((s.xdirps, DIR_X), (s.ydirps, DIR_Y), (s.zdirps, DIR_Z))
    gb = [grads[m] for m in PHI_BLOCK]
    for q, f in enumerate((s.species[0], s.v)):
        for j, (dirps, direction) in enumerate(dirs):
            b.tds_apply(gb[3 * q + j], f, dirps.der1st, direction)
    saved = [al.get_block(DIR_X, VERT) for _ in range(6)]
    for d, g in zip(saved, gb):
        b.veccopy(d, g)
    acc = [al.get_block(DIR_X, VERT) for _ in range(9)]
    for f in acc:
        f.fill(0.0)
    row = torch.zeros(2, dtype=torch.float64, device=b.device)
    ms, times = ctypes.c_float(), {1: [], 2: [], "stats": []}
    for i in range(args.stat_warmup + args.stat_iters):
        for ns in (1, 2):
            for d, g in zip(saved, gb):
                b.veccopy(g, d)
            _lib.check(b.lib.x3d_timer_start(b.h))
            b.les_scalar_flux(grads[NUT_BLOCK], gb[:3 * ns], [1.0 / 0.85, 1.0 / 0.4][:ns], row.data_ptr())
            _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
            if i >= args.stat_warmup:
                times[ns].append(ms.value)
        _lib.check(b.lib.x3d_timer_start(b.h))
        b.stats_update_uvw(s.u, s.v, s.w, acc, 0.125)
        _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
        if i >= args.stat_warmup:
            times["stats"].append(ms.value)
    t_stats = spread(times["stats"])
    nbytes = 21 * rb * n ** 3
    emit(dict({"op": "x3d_stats_update_uvw in the loop of x3d_les_scalar_flux (3 blocks read, 9 read and written)",
               "bytes_per_dof": 21 * rb, "TBs": nbytes / t_stats["ms_median"] / 1e9,
               "ceiling": nbytes / t_stats["ms_median"] / 1e6 / 6200.0}, **t_stats))
    for ns in (1, 2):
        t = spread(times[ns])
        dof = (1 + 6 * ns) * rb
        nbytes = dof * n ** 3
        emit(dict({"op": "x3d_les_scalar_flux, ns = %d: both launches (%d blocks read, %d written)" % (ns, 1 + 3 * ns, 3 * ns),
                   "bytes_per_dof": dof, "TBs": nbytes / t["ms_median"] / 1e9, "ceiling": nbytes / t["ms_median"] / 1e6 / 6200.0,
                   "row_pitch": b.padded_dims[0]}, **t))
        limit = 1.25 * (dof / (21.0 * rb)) * t_stats["ms_median"]
        emit({"op": "gate: t_flux <= 1.25 (%d / %d) t_stats_update, ns = %d" % (dof, 21 * rb, ns), "flux_ms_median": t["ms_median"],
              "stats_update_ms_median": t_stats["ms_median"], "limit_ms": limit, "ratio_to_limit": t["ms_median"] / limit,
              "passed": bool(t["ms_median"] <= limit)})
    for f in grads + saved + acc:
        al.release_block(f)
    # (e) a whole Les.add with one species, from call to return (wall clock around a device sync)
    d = [al.get_block(DIR_X, VERT) for _ in range(4)]
    for f in d:
        f.fill(0.0)
    s0 = b.sync_count()
    t = spread(timed_wall(args, b, lambda: les.add(d[0], d[1], d[2], [d[3]], list(s.species))))
    emit(dict({"op": "Les.add, wale, one species: 9 + 3 gradients, stress, flux, 9 + 3 accumulated derivatives (wall clock)",
               "stream_syncs_per_call": (b.sync_count() - s0) / float(args.stat_warmup + args.stat_iters),
               "monitor": les.monitor()}, **t))
    del case, s, b, al, les, grads, gb, saved, acc, d
    torch.cuda.empty_cache()
    # (f) 20 steps: LES without species, one species without LES, LES with one species (the first two are the parent's paths)
    setups = (("LES (wale) without species", 0, LesConfig(model="wale")), ("one species without LES", 1, None),
              ("LES (wale, prt = 0.85) with one species", 1, LesConfig(model="wale", prt=0.85)))
    res = {}
    for name, nspec, cfg in setups:
        case = make_tgv(n, fused=True, **(dict(n_species=1, pr_species=[0.7]) if nspec else {}))
        if nspec:
            case.solver.species[0].set_data_loc(VERT)
            case.solver.backend.veccopy(case.solver.species[0], case.solver.u)
        if cfg is not None:
            case.solver.les = Les(case.solver, cfg)
        case.run(n_iters=3)
        case.solver.backend.sync()
        t0 = time.perf_counter()
        case.run(n_iters=23)
        case.solver.backend.sync()
        res[name] = (time.perf_counter() - t0) * 1e3
        emit({"op": "TGV, fused, RK3: 20 steps, " + name, "wall_ms": res[name], "ms_per_step": res[name] / 20.0})
        del case
        torch.cuda.empty_cache()
    a, c, both = (res[name] for name, _, _ in setups)
    emit({"op": "TGV, fused, RK3: 20 steps: what a species adds to an LES step, and the model to a step with a species",
          "added_ms_per_step_species_to_les": (both - a) / 20.0, "added_ms_per_step_les_to_species": (both - c) / 20.0})


def bench_particles(args):
    """one JSON line per measurement of the "particles" family, printed and appended to profiles/particles.jsonl"""
    import ctypes
    import tempfile

    import torch
    from x3d2_amd import _lib, make_tgv
    from x3d2_amd.particles import Particles, ParticlesConfig, seed_uniform
    from x3d2_amd.probes import Probes, ProbesConfig
    n, rb = args.snap_n, 4 if _lib.SINGLE else 8
    tmp = tempfile.mkdtemp(prefix="x3d_particles_")
    out_path = os.path.join(ROOT, "profiles", "particles.jsonl")

    def emit(row):
        row = dict({"family": "particles", "n": n, "real_bytes": rb}, **row)
        line = json.dumps(row)
        print(line, flush=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")

    # (a) the launches alone, on the velocity of a TGV run three steps old
    case = make_tgv(n, fused=True)
    s = case.solver
    b = s.backend
    case.run(n_iters=3)
    for log2 in (() if args.particles_part == "mp" else (16, 20, 22)):
        npart = 1 << log2
        x0 = seed_uniform(s.mesh, npart, seed=1)
        for order in (2, 4):
            for tau in (0.0, 20.0 * float(s.dt)):
                p = Particles(s, ParticlesConfig(x0, order=order, tau_p=tau))
                kind = "inertial" if tau else "tracers"
                fetched = order ** 3 * 3 * rb  # field bytes a particle's stencils ask for
                for state in ("random order", "sorted"):
                    if state == "sorted":
                        _lib.check(b.lib.x3d_timer_start(b.h))
                        p.sort()
                        ms = ctypes.c_float()
                        _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
                        emit({"op": "x3d_particles_sort from random order: keys + radix sort + gather (one sample)", "particles": npart,
                              "order": order, "kind": kind, "ms": ms.value})
                    t = spread(timed_events(args, b, lambda: p.advance(s.u, s.v, s.w, s.dt)))
                    emit(dict({"op": "x3d_particles_advance, %s" % state, "particles": npart, "order": order, "kind": kind,
                               "particles_per_s": npart / t["ms_median"] * 1e3, "fetched_bytes_per_particle": fetched,
                               "fetched_GBs": npart * fetched / t["ms_median"] / 1e6}, **t))
                t = spread(timed_events(args, b, p.sort))
                emit(dict({"op": "x3d_particles_sort of a sorted state: keys + radix sort + gather", "particles": npart, "order": order,
                           "kind": kind}, **t))
                del p
    bench_particles_mp(args, emit, s)
    if args.particles_part == "mp":
        return
    pts = seed_uniform(s.mesh, 4096, seed=2)
    pr = Probes(s, ProbesConfig(pts, prefix=os.path.join(tmp, "probes")))
    row = torch.zeros(3 * 4096, dtype=torch.float64, device=b.device)
    t = spread(timed_events(args, b, lambda: b.probe_sample(pr.h, s.u, s.v, s.w, row.data_ptr())))
    emit(dict({"op": "x3d_probe_sample on the same box, 4096 probes"}, **t))
    del case, s, b, pr, row
    torch.cuda.empty_cache()
    # (b) the default sort_every: 64 steps with 2^20 tracers seeded in random order; HIP events around Particles.update
    for m in (0, 1, 8, 64):
        case = make_tgv(n, fused=True)
        s = case.solver
        b = s.backend
        p = Particles(s, ParticlesConfig(seed_uniform(s.mesh, 1 << 20, seed=1), sort_every=m))
        ms, times = ctypes.c_float(), []
        for it in range(1, 65):
            case.step(it)
            s.current_iter = it
            s.flush_grad()
            _lib.check(b.lib.x3d_timer_start(b.h))
            p.update(it)
            _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
            times.append(ms.value)
        emit({"op": "Particles.update over 64 fused TGV steps, 2^20 order-4 tracers", "sort_every": m,
              "particle_ms_per_step": float(np.mean(times)), "ms_median": float(np.median(times)), "ms_max": float(max(times))})
        del case, s, b, p
        torch.cuda.empty_cache()
    # (c) 20 steps: nothing attached (the parent's path), probes at every step (gives up the deferral too), 2^20 order-4 tracers
    res = {}
    for what in ("nothing", "probes", "particles"):
        case = make_tgv(n, fused=True)
        s = case.solver
        if what == "probes":
            case.probes = Probes(s, ProbesConfig(pts, prefix=os.path.join(tmp, "probes20")))
        if what == "particles":
            case.particles = Particles(s, ParticlesConfig(seed_uniform(s.mesh, 1 << 20, seed=1), sort_every=0))
        case.run(n_iters=3)
        s.backend.sync()
        t0 = time.perf_counter()
        case.run(n_iters=23)
        s.backend.sync()
        res[what] = (time.perf_counter() - t0) * 1e3
        del case, s
        torch.cuda.empty_cache()
    for what in ("probes", "particles"):
        emit({"op": "TGV, fused, RK3: 20 steps, %s" % what, "wall_ms_without": res["nothing"], "wall_ms_with": res[what],
              "ms_per_step_without": res["nothing"] / 20.0, "added_ms_per_step": (res[what] - res["nothing"]) / 20.0})


def bench_particles_mp(args, emit, s):
    """(d) of the "particles" family: the launches of a several-rank advance beside the fused one-rank launch, in one loop"""
    import ctypes

    import torch
    from x3d2_amd import _lib
    from x3d2_amd.diagnostics import global_vert_coords
    from x3d2_amd.particles import DP, Particles, ParticlesConfig, seed_uniform
    b, m, lib = s.backend, s.mesh, s.backend.lib
    n, rb, npart, order, gh = [int(v) for v in m.vert_dims], 4 if _lib.SINGLE else 8, 1 << 20, 4, 2
    x0 = seed_uniform(m, npart, seed=1)
    fused = Particles(s, ParticlesConfig(x0, order=order, sort_every=0))
    # the box as rank 0 of two z slabs: the z table runs on over a second box, the period doubles
    coords = [np.ascontiguousarray(global_vert_coords(m, d), dtype=np.float64) for d in range(3)]
    coords[2] = np.concatenate([coords[2], coords[2] + float(m.L[2])])
    prm, dc = _lib.ParticlesParams(), _lib.ParticlesDecomp()
    prm.n, prm.order, prm.wall, prm.tau = 2 * npart, order, 0, 0.0
    for d in range(3):
        prm.periodic[d], prm.uniform[d], prm.L[d] = 1, 1, float(m.L[d]) * (2 if d == 2 else 1)
        prm.coords[d] = coords[d].ctypes.data_as(DP)
        dc.nglobal[d], dc.offset[d], dc.nlocal[d], dc.nproc[d], dc.rank[d] = n[d] * (2 if d == 2 else 1), 0, n[d], 2 if d == 2 else 1, 0
    dc.capacity, dc.mig_capacity = ParticlesConfig(np.zeros((2 * npart, 3))).capacities(2)
    ids = np.arange(npart, dtype=np.int32)
    xt = np.ascontiguousarray(x0.T)
    h = ctypes.c_void_p()
    _lib.check(lib.x3d_particles_mp_create(b.h, ctypes.byref(prm), ctypes.byref(dc), xt.ctypes.data_as(DP), None,
                                           ids.ctypes.data_as(_lib.c_int_p), npart, ctypes.byref(h)))
    real = torch.float64 if rb == 8 else torch.float32
    nr = n[1] + 1 + gh
    ghost_lo = torch.zeros(3 * gh * nr * n[0], dtype=real, device=b.device)  # to pprev = what pnext sends = this rank's own
    ghost_hi = torch.zeros(3 * nr * n[0], dtype=real, device=b.device)
    mig = [torch.zeros(1 + 13 * dc.mig_capacity, dtype=torch.float64, device=b.device) for _ in range(2)]
    fields = (s.u.ptr, s.v.ptr, s.w.ptr, b._dims(0))
    dt = float(s.dt)

    def ghosts():
        _lib.check(lib.x3d_particles_mp_ghost_pack(b.h, h, 3, *fields, ghost_lo.data_ptr(), ghost_hi.data_ptr()))
        _lib.check(lib.x3d_particles_mp_ghost_unpack(b.h, h, 3, ghost_hi.data_ptr(), ghost_lo.data_ptr()))

    def migrate():
        _lib.check(lib.x3d_particles_mp_emigrate(b.h, h, 3, mig[0].data_ptr(), mig[1].data_ptr()))
        _lib.check(lib.x3d_particles_mp_immigrate(b.h, h, 3, mig[1].data_ptr(), mig[0].data_ptr()))

    ghosts()
    _lib.check(lib.x3d_particles_mp_prime(b.h, h, *fields))
    stages = [("x3d_particles_advance (fused, one rank)", lambda: fused.advance(s.u, s.v, s.w, dt)),
              ("x3d_particles_mp_move", lambda: _lib.check(lib.x3d_particles_mp_move(b.h, h, dt))),
              ("x3d_particles_mp_emigrate + immigrate (z)", migrate),
              ("x3d_particles_mp_ghost_pack + unpack (z)", ghosts),
              ("x3d_particles_mp_sample", lambda: _lib.check(lib.x3d_particles_mp_sample(b.h, h, *fields)))]
    ms, times = ctypes.c_float(), {name: [] for name, _ in stages}
    for i in range(args.stat_warmup + args.stat_iters):
        for name, fn in stages:
            _lib.check(lib.x3d_timer_start(b.h))
            fn()
            _lib.check(lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
            if i >= args.stat_warmup:
                times[name].append(ms.value)
    q = (ctypes.c_int * 2)()
    _lib.check(lib.x3d_particles_mp_query(b.h, h, q))
    t = {name: spread(v) for name, v in times.items()}
    face_bytes = (ghost_lo.numel() + ghost_hi.numel()) * rb
    for name, _ in stages:
        row = {"op": name + ", random order", "particles": npart, "order": order, "kind": "tracers"}
        if "ghost" in name:
            row["face_bytes_per_direction"] = face_bytes
        if "migrate" in name or "emigrate" in name:
            row["message_bytes"] = 2 * mig[0].numel() * 8
        emit(dict(row, **t[name]))
    adv, split = t[stages[0][0]]["ms_median"], t[stages[1][0]]["ms_median"] + t[stages[4][0]]["ms_median"]
    emit({"op": "gate: t_move + t_sample <= 1.25 t_advance", "particles": npart, "order": order, "kind": "tracers", "ms_advance": adv,
          "ms_move_plus_sample": split, "ratio": split / adv, "passed": bool(split <= 1.25 * adv),
          "added_ms_per_step_migrate": t[stages[2][0]]["ms_median"], "added_ms_per_step_ghosts": t[stages[3][0]]["ms_median"],
          "residents_after": int(q[0]), "flags_after": int(q[1])})
    _lib.check(lib.x3d_particles_destroy(h))
    del fused


def bench_scalars(args):
    """one JSON line per measurement of the "scalars" family, printed and appended to profiles/scalars.jsonl"""
    import ctypes

    import torch
    from x3d2_amd import _lib, make_tgv
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.scalars import Scalars, ScalarsConfig
    n, rb = args.snap_n, 4 if _lib.SINGLE else 8
    out_path = os.path.join(ROOT, "profiles", "scalars.jsonl")

    def emit(row):
        row = dict({"family": "scalars", "n": n, "real_bytes": rb}, **row)
        line = json.dumps(row)
        print(line, flush=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")

    def alternating(fns):
        """HIP-event ms of each fn in turn, --stat-iters rounds after --stat-warmup: both see the same machine state"""
        ms, times = ctypes.c_float(), [[] for _ in fns]
        for i in range(args.stat_warmup + args.stat_iters):
            for k, fn in enumerate(fns):
                _lib.check(b.lib.x3d_timer_start(b.h))
                fn()
                _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
                if i >= args.stat_warmup:
                    times[k].append(ms.value)
        return [spread(x) for x in times]

    case = make_tgv(n, fused=True, n_species=3, pr_species=[1.0, 0.7, 2.0])
    s = case.solver
    b, al = s.backend, s.backend.allocator
    for i, f in enumerate(s.species):
        f.set_data_loc(VERT)
        b.veccopy(f, (s.u, s.v, s.u)[i])
    d = [al.get_block(DIR_X, VERT) for _ in range(6)]
    for f in d:
        f.fill(0.0)
    dof = float(n) ** 3
    rate = lambda nbytes, t: {"bytes_per_dof": nbytes, "TBs": nbytes * dof / t["ms_median"] / 1e9,
                              "ceiling": nbytes * dof / t["ms_median"] / 1e6 / 6200.0}
    # (a) ns = 1, up = y: phi read, dv read and written -- what x3d_vecadd moves on the same blocks
    one = lambda: b.scalars_couple(d[0:3], d[3:4], [s.u, s.v, s.w], s.species[0:1], (0, 1, 0), [1.0], [0.5])
    t_c, t_v = alternating([one, lambda: b.vecadd(1.0, s.species[0], 1.0, d[1])])
    emit(dict({"op": "x3d_scalars_couple, ns = 1, up = y (phi read, dv read and written)", "row_pitch": b.padded_dims[0]},
              **rate(3 * rb, t_c), **t_c))
    emit(dict({"op": "x3d_vecadd on the same blocks"}, **rate(3 * rb, t_v), **t_v))
    limit = 1.15 * t_v["ms_median"]
    emit({"op": "gate: t_couple(ns = 1) <= 1.15 t_vecadd", "couple_ms_median": t_c["ms_median"], "couple_ms_q1_q3": [t_c["ms_q1"], t_c["ms_q3"]],
          "vecadd_ms_median": t_v["ms_median"], "vecadd_ms_q1_q3": [t_v["ms_q1"], t_v["ms_q3"]], "limit_ms": limit,
          "ratio": t_c["ms_median"] / t_v["ms_median"], "passed": bool(t_c["ms_median"] <= limit)})
    # (b) ns = 3, an oblique up, G != 0 on every species: 3 phi + 2 x 2 d + 3 vel + 2 x 3 dphi = 16 streams, next to the vecadd
    # calls that compose the same terms (2 x 3 buoyancy + 6 advection: 12 calls of 3 streams)
    up, ri, ref = (0.6, 0.8, 0.0), [1.0, 0.5, -0.25], [0.5, 0.0, 0.1]
    grad = [(0.1, 0.2, 0.3), (0.0, 1.0, 0.0), (0.3, 0.0, -0.1)]
    three = lambda: b.scalars_couple(d[0:3], d[3:6], [s.u, s.v, s.w], s.species, up, ri, ref, grad)

    def composed():
        for i in (0, 1):
            for k in range(3):
                b.vecadd(up[i] * ri[k], s.species[k], 1.0, d[i])  # (the reference values: one field_shift more per component)
        for k in range(3):
            for i, vel in enumerate((s.u, s.v, s.w)):
                if grad[k][i] != 0.0:
                    b.vecadd(-grad[k][i], vel, 1.0, d[3 + k])

    t_c3, t_v3 = alternating([three, composed])
    emit(dict({"op": "x3d_scalars_couple, ns = 3, up = (0.6, 0.8, 0), G != 0 (16 streams)"}, **rate(16 * rb, t_c3), **t_c3))
    emit(dict({"op": "the 12 x3d_vecadd calls that compose the same terms (36 streams)"}, **rate(36 * rb, t_v3), **t_v3))
    # (c) the plane sums, ns = 1, next to the statistics' on u, v, w
    nk = n
    z = lambda m: torch.zeros(m, dtype=_lib.torch_real(), device=b.device)
    sums, mm, sums9 = z(5 * nk), z(2), z(9 * nk)
    t_p, t_s = alternating([lambda: b.scalars_profile_sums(s.u, s.v, s.w, s.species[0:1], 2, sums, mm),
                            lambda: b.stats_profile_sums(s.u, s.v, s.w, 2, sums9)])
    emit(dict({"op": "x3d_scalars_profile_sums, ns = 1, dir_keep = 2 (u, v, w, phi read)"}, **rate(4 * rb, t_p), **t_p))
    emit(dict({"op": "x3d_stats_profile_sums, dir_keep = 2 (u, v, w read)"}, **rate(3 * rb, t_s), **t_s))
    for f in d:
        al.release_block(f)
    del case, s, b, al, d
    torch.cuda.empty_cache()
    # (d) 20 fused RK3 steps with one passive species against the same run with ri = 1: what giving up the deferred branch costs
    res = {}
    for ri1 in (0.0, 1.0):
        case = make_tgv(n, fused=True, n_species=1)
        s = case.solver
        s.species[0].set_data_loc(VERT)
        s.backend.veccopy(s.species[0], s.u)
        s.scalars = Scalars(s, ScalarsConfig(ri=[ri1], up=(0, 0, 1)))
        case.run(n_iters=3)
        s.backend.sync()
        t0 = time.perf_counter()
        case.run(n_iters=23)
        s.backend.sync()
        res[ri1] = (time.perf_counter() - t0) * 1e3
        del case, s
        torch.cuda.empty_cache()
    emit({"op": "TGV, fused, RK3, one species: 20 steps, ri = 0 (deferred branch) against ri = 1 (stored derivatives + coupling)",
          "wall_ms_passive": res[0.0], "wall_ms_active": res[1.0], "ms_per_step_passive": res[0.0] / 20.0,
          "added_ms_per_step": (res[1.0] - res[0.0]) / 20.0})


def bench_forcing(args):
    """one JSON line per measurement of the "forcing" family, printed and appended to profiles/forcing.jsonl"""
    import ctypes

    import torch
    from x3d2_amd import _lib, make_hit
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.forcing import Forcing, ForcingConfig
    n, rb = args.snap_n, 4 if _lib.SINGLE else 8
    out_path = os.path.join(ROOT, "profiles", "forcing.jsonl")

    def emit(row):
        row = dict({"family": "forcing", "n": n, "real_bytes": rb}, **row)
        line = json.dumps(row)
        print(line, flush=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")

    def alternating(fns):
        """HIP-event ms of each fn in turn, --stat-iters rounds after --stat-warmup: both see the same machine state"""
        ms, times = ctypes.c_float(), [[] for _ in fns]
        for i in range(args.stat_warmup + args.stat_iters):
            for k, fn in enumerate(fns):
                _lib.check(b.lib.x3d_timer_start(b.h))
                fn()
                _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
                if i >= args.stat_warmup:
                    times[k].append(ms.value)
        return [spread(x) for x in times]

    case = make_hit(n, fused=True)
    s = case.solver
    b, al = s.backend, s.backend.allocator
    d = [al.get_block(DIR_X, VERT) for _ in range(3)]
    for f in d:
        f.fill(0.0)
    dof = float(n) ** 3
    rate = lambda nbytes, t: {"bytes_per_dof": nbytes, "TBs": nbytes * dof / t["ms_median"] / 1e9,
                              "ceiling": nbytes * dof / t["ms_median"] / 1e6 / 6200.0}
    sums9 = torch.zeros(9 * n, dtype=_lib.torch_real(), device=b.device)
    profile = lambda: b.stats_profile_sums(s.u, s.v, s.w, 2, sums9)

    def three_vecadd():
        for f in d:  # (x = y: one read and one write of each block, the bytes the synthesis moves)
            b.vecadd(1e-3, f, 1.0, f)

    for k_hi, gated in ((2.5, True), (4.5, False)):
        frc = Forcing(s, ForcingConfig(scheme="power", power=0.1, k_hi=k_hi))
        frc.add(d[0], d[1], d[2], s.u, s.v, s.w)  # (the coefficients the synthesis is timed with)
        tag = "M = %d" % frc.M[0]
        t_a, t_p = alternating([lambda: frc.project(s.u, s.v, s.w), profile])
        emit(dict({"op": "x3d_forcing_project, %s (u, v, w read)" % tag, "row_pitch": b.padded_dims[0]}, **rate(3 * rb, t_a), **t_a))
        emit(dict({"op": "x3d_stats_profile_sums, dir_keep = 2, on the same fields"}, **rate(3 * rb, t_p), **t_p))
        t_c, t_v = alternating([lambda: frc.synthesise(d[0], d[1], d[2]), three_vecadd])
        emit(dict({"op": "x3d_forcing_synth, %s (three derivative blocks read and written)" % tag}, **rate(6 * rb, t_c), **t_c))
        emit(dict({"op": "three x3d_vecadd calls on the same blocks, x = y (three blocks read and written)"}, **rate(6 * rb, t_v), **t_v))
        for name, t, y, what in (("t_A <= 1.25 t_profile_sums", t_a, t_p, "project"), ("t_C <= 1.25 t_3vecadd", t_c, t_v, "synth")):
            row = {"op": ("gate: " if gated else "reported, no gate: ") + name + ", " + tag, what + "_ms_median": t["ms_median"],
                   what + "_ms_q1_q3": [t["ms_q1"], t["ms_q3"]], "yardstick_ms_median": y["ms_median"],
                   "yardstick_ms_q1_q3": [y["ms_q1"], y["ms_q3"]], "ratio": t["ms_median"] / y["ms_median"]}
            if gated:
                row.update(limit_ms=1.25 * y["ms_median"], passed=bool(t["ms_median"] <= 1.25 * y["ms_median"]))
            emit(row)
        t_add = spread(timed_events(args, b, lambda: frc.add(d[0], d[1], d[2], s.u, s.v, s.w)))
        emit(dict({"op": "Forcing.add as a whole, %s" % tag, "row": frc.row()}, **t_add))
        del frc
    for f in d:
        al.release_block(f)
    # 20 fused RK3 steps without and with the forcing, on the same case
    res = {}
    for forced in (False, True):
        s.forcing = Forcing(s, ForcingConfig(scheme="power", power=0.1, k_hi=2.5)) if forced else None
        start = s.current_iter
        case.run(n_iters=start + 3)
        b.sync()
        t0 = time.perf_counter()
        case.run(n_iters=start + 23)
        b.sync()
        res[forced] = (time.perf_counter() - t0) * 1e3
    emit({"op": "make_hit, fused, RK3: 20 steps without and with the band forcing (k_hi = 2.5)", "wall_ms_plain": res[False],
          "wall_ms_forced": res[True], "ms_per_step_plain": res[False] / 20.0, "added_ms_per_step": (res[True] - res[False]) / 20.0,
          "row": s.forcing.row()})


def bench_feedback(args):
    """one JSON line per measurement of the "feedback" family, printed and appended to profiles/feedback.jsonl"""
    import ctypes

    from x3d2_amd import _lib, make_hit
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.particles import Particles, ParticlesConfig, mass_for_loading, seed_uniform
    n, rb = args.snap_n, 4 if _lib.SINGLE else 8
    out_path = os.path.join(ROOT, "profiles", "feedback.jsonl")

    def emit(row):
        row = dict({"family": "feedback", "n": n, "real_bytes": rb}, **row)
        line = json.dumps(row)
        print(line, flush=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")

    def alternating(fns):
        """HIP-event ms of each fn in turn, --stat-iters rounds after --stat-warmup: both see the same machine state"""
        ms, times = ctypes.c_float(), [[] for _ in fns]
        for i in range(args.stat_warmup + args.stat_iters):
            for k, fn in enumerate(fns):
                _lib.check(b.lib.x3d_timer_start(b.h))
                fn()
                _lib.check(b.lib.x3d_timer_stop_ms(b.h, ctypes.byref(ms)))
                if i >= args.stat_warmup:
                    times[k].append(ms.value)
        return [spread(x) for x in times]

    case = make_hit(n, fused=True)
    s = case.solver
    b, al = s.backend, s.backend.allocator
    tau = 20.0 * float(s.dt)

    def particles(npart):
        cfg = ParticlesConfig(seed_uniform(s.mesh, npart, seed=1), tau_p=tau, two_way=True, mass=mass_for_loading(s.mesh, npart, 0.2),
                              v0=np.zeros((npart, 3)))
        return Particles(s, cfg)

    npart = 1 << 20
    p = particles(npart)
    fb = p.feedback
    counts, _, _ = fb.records()
    d = [al.get_block(DIR_X, VERT) for _ in range(3)]
    for f in d:
        f.fill(0.0)

    def three_vecadd():
        for f in d:  # (x = y: one read and one write of each block)
            b.vecadd(1e-3, f, 1.0, f)

    t_add, t_v = alternating([lambda: fb.add(d[0], d[1], d[2]), three_vecadd])
    emit(dict({"op": "Feedback.add, eight passes, 2^20 particles", "particles": npart, "occupied_cells": int(counts[8]),
               "cells_by_colour": [int(counts[c + 1] - counts[c]) for c in range(8)]}, **t_add))
    emit(dict({"op": "three x3d_vecadd calls on the same blocks, x = y"}, **t_v))
    emit({"op": "gate: t_add <= t_3vecadd", "add_ms_median": t_add["ms_median"], "add_ms_q1_q3": [t_add["ms_q1"], t_add["ms_q3"]],
          "yardstick_ms_median": t_v["ms_median"], "yardstick_ms_q1_q3": [t_v["ms_q1"], t_v["ms_q3"]],
          "ratio": t_add["ms_median"] / t_v["ms_median"], "passed": bool(t_add["ms_median"] <= t_v["ms_median"])})
    for f in d:
        al.release_block(f)
    t_b, t_s, t_a = alternating([fb.build, p.sort, lambda: p.advance(s.u, s.v, s.w, 1e-9)])  # (dt tiny: the particles stay)
    emit(dict({"op": "record build (keys, sort, marks, sort, offsets, records), 2^20 particles", "particles": npart}, **t_b))
    emit(dict({"op": "Particles.sort, on the same state"}, **t_s))
    emit(dict({"op": "x3d_particles_advance, order 4, on the same state"}, **t_a))
    s.particle_feedback = None
    del p, fb
    big = particles(1 << 22)
    (t_b4,) = alternating([big.feedback.build])
    emit(dict({"op": "record build, 2^22 particles", "particles": 1 << 22, "occupied_cells": int(big.feedback.records()[0][8])}, **t_b4))
    s.particle_feedback = None
    del big
    # 20 fused RK3 steps with the particles one-way and two-way, each on a case of its own
    res = {}
    del case, s, b, al
    for two_way in (False, True):
        case = make_hit(n, fused=True)
        s = case.solver
        extra = dict(two_way=True, mass=mass_for_loading(s.mesh, npart, 0.2)) if two_way else {}
        case.particles = Particles(s, ParticlesConfig(seed_uniform(s.mesh, npart, seed=1), tau_p=tau, v0=np.zeros((npart, 3)), **extra))
        case.run(n_iters=3)
        s.backend.sync()
        t0 = time.perf_counter()
        case.run(n_iters=23)
        s.backend.sync()
        res[two_way] = (time.perf_counter() - t0) * 1e3
        del case, s
    emit({"op": "make_hit, fused, RK3: 20 steps with 2^20 inertial particles, one-way and two-way", "wall_ms_one_way": res[False],
          "wall_ms_two_way": res[True], "ms_per_step_one_way": res[False] / 20.0, "added_ms_per_step": (res[True] - res[False]) / 20.0})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="256,512,1024")  # the sizes of perf_cuda_tridiag
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--family", default="all", choices=("all", "operators", "stats", "ibm", "snapshot", "checkpoint", "spectra", "diagnostics", "loads",
                                                               "budgets", "les", "particles", "scalars", "forcing", "feedback"))
    ap.add_argument("--snap-n", type=int, default=512)
    ap.add_argument("--stat-iters", type=int, default=30)
    ap.add_argument("--stat-warmup", type=int, default=5)
    ap.add_argument("--particles-part", default="all", choices=("all", "mp"))  # family particles: everything, or (d) alone
    args = ap.parse_args()
    if args.family in ("all", "stats"):
        bench_stats(args)
    if args.family in ("all", "ibm"):
        bench_ibm(args)
    if args.family == "snapshot":
        bench_snapshot(args)
    if args.family == "checkpoint":
        bench_checkpoint(args)
    if args.family == "spectra":
        bench_spectra(args)
    if args.family == "diagnostics":
        bench_diagnostics(args)
    if args.family == "budgets":
        bench_budgets(args)
    if args.family == "loads":
        bench_loads(args)
    if args.family == "les":
        bench_les(args)
    if args.family == "particles":
        bench_particles(args)
    if args.family == "scalars":
        bench_scalars(args)
    if args.family == "forcing":
        bench_forcing(args)
    if args.family == "feedback":
        bench_feedback(args)
    if args.family in ("stats", "ibm", "snapshot", "checkpoint", "spectra", "diagnostics", "budgets", "loads", "les", "particles", "scalars",
                       "forcing", "feedback"):
        return
    import torch
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.solver import Solver, SolverConfig
    twopi = 6.283185307179586
    per = ("periodic",) * 2
    for n in (int(v) for v in args.n.split(",")):
        for d, dname in ((1, "x"), (2, "y"), (3, "z")):
            dims = [512, 512, 512]
            dims[d - 1] = n
            mesh = Mesh(tuple(dims), (1, 1, 1), (twopi,) * 3, per, per, per)
            s = Solver(HipBackend(mesh), mesh, SolverConfig(poisson_solver_type="CG", fused=True))
            b, al = s.backend, s.backend.allocator
            dirps = (s.xdirps, s.ydirps, s.zdirps)[d - 1]
            nx, ny, nz = dims
            idx = [np.arange(m) for m in (nz, ny, nx)]
            grid = np.meshgrid(*idx, indexing="ij")[3 - d]
            dx = twopi / n
            for f, fn in ((s.u, np.sin), (s.v, np.cos)):
                f.set_data_loc(VERT)
                b.set_field_data(f, fn(grid * dx))
            s.w.set_data_loc(VERT)
            b.set_field_data(s.w, np.cos(grid * dx))
            out = [al.get_block(DIR_X, VERT) for _ in range(3)]
            dof = nx * ny * nz

            def timed(fn):
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / args.iters

            t = timed(lambda: b.tds_apply(out[0], s.u, dirps.der2nd, d))
            print(json.dumps({"op": "tds_solve second-deriv compact6 periodic", "dir": dname, "n": n,
                              "pencils": dof // n, "ms": t * 1e3, "GBs_algorithmic_16B": 16 * dof / t / 1e9,
                              "GBs_reference_convention_48B": 48 * dof / t / 1e9}))
            # the three components of one direction (advecting velocity = component d)
            t = timed(lambda: b.transeq_dir(d, out[0], out[1], out[2], s.u, s.v, s.w, 1.0, dirps, accumulate=False))
            print(json.dumps({"op": "transeq (3 components, fused subs)", "dir": dname, "n": n,
                              "pencils": dof // n, "ms": t * 1e3, "ms_per_component": t * 1e3 / 3,
                              "GBs_algorithmic_64B": 64 * dof / t / 1e9,
                              "GBs_reference_convention_384B": 384 * dof / t / 1e9}))
            del s, b, al, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
