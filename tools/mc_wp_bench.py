"""Motion compensation with and without explicit weighted prediction on one batch: 16 pictures of 2160p, 8 bit, the PU mix of the
random-access leg (thevc_amd/workload.make_pus, two references, half of the units on both lists), cell-map schedule.

  python tools/mc_wp_bench.py [--parent OLDER_LIBHMX_SO] [--repeats N] [--out profiles/mc_wp_bench.txt]

The driver starts one child process per step, each under a time limit, and stops at the first one that fails: this build, then
(with --parent) the older build loaded through HMX_LIB_PATH, alternating twice.  A child times, in ONE process and interleaved,
hmx_batch_motionCompensation_multi and (where the library has it) hmx_batch_motionCompensation_wp_multi with HIP events around
INNER calls, after a warm-up of both; every line is the median of the repeats with their min..max, which is the spread the
comparison has to be read against.  It also prints a checksum of the unweighted prediction (equal across builds) and checks that
the weighted call with weights 1 << d and no offsets reproduces it."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, W, H, M, NP, INNER = 8, 3840, 2160, 80, 16, 10


def child(repeats):
    from thevc_amd import capi, workload
    ctx, L = capi.Context(bit_depth=B), capi.lib()
    have_wp = hasattr(L, "hmx_batch_motionCompensation_wp_multi")
    refs = [capi.DevPicture(ctx, W, H, M, M).upload(workload.make_planes(i, W, H, B, "texture")) for i in range(2)]
    for r in refs:
        ctx._chk(L.hmx_pic_extend_border(ctx.h, C.byref(r.as_pic()), W, H, M, M))
    pus = workload.make_pus(3, W, H, n_refs=2, bi_frac=0.5)
    d_pus = ctx.to_device(pus)
    pred = [capi.DevPicture(ctx, W, H).zero() for _ in range(NP)]
    ref_arr, a_pred, mc = (capi.Pic * 2)(*[r.as_pic() for r in refs]), (capi.Pic * NP)(), (capi.McJob * NP)()
    for q in range(NP):
        a_pred[q] = pred[q].as_pic()
        mc[q].d_pus, mc[q].n_pus, mc[q].refs, mc[q].n_refs = d_pus.ptr, len(pus), ref_arr, 2
        mc[q].dst, mc[q].pic_w, mc[q].pic_h = C.pointer(a_pred[q]), W, H
    calls = {"unweighted": lambda: ctx._chk(L.hmx_batch_motionCompensation_multi(ctx.h, NP, mc))}
    if have_wp:
        rng = np.random.default_rng(9)

        def tables(unit):
            out = []
            for _ in range(NP):
                t = np.zeros((2, 2), capi.WP_DTYPE)
                d = rng.integers(0, 8, 3)
                t["log2_denom"] = d
                t["weight"] = (1 << d) if unit else (1 << d) + rng.integers(-(1 << d) // 2, (1 << d) // 2 + 1, (2, 2, 3))
                t["offset"] = 0 if unit else rng.integers(-20, 21, (2, 2, 3))
                out.append((t[0], t[1]))
            return capi.mc_wp_array(out)
        fade, unit = tables(False), tables(True)
        calls["weighted"] = lambda: ctx._chk(L.hmx_batch_motionCompensation_wp_multi(ctx.h, NP, mc, fade[0]))

    def crc():
        ctx.sync()
        return zlib.crc32(b"".join(p.tobytes() for q in (0, NP - 1) for p in pred[q].download()))

    calls["unweighted"]()
    print(f"{NP} pictures {W}x{H}, {B} bit, {len(pus)} units a picture ({int((pus['ref1'] != 255).sum())} on both lists)")
    plain = crc()
    print(f"unweighted prediction, pictures 0 and {NP - 1}: crc32 {plain:08x}")
    if have_wp:
        ctx._chk(L.hmx_batch_motionCompensation_wp_multi(ctx.h, NP, mc, unit[0]))
        same = crc() == plain
        print(f"weighted call with weights 1 << d, offsets 0 gives the unweighted prediction: {same}")
        assert same
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        ctx._chk(L.hmx_event_create(ctx.h, C.byref(e)))
    for f in calls.values():  # warm-up of every kernel that is timed
        for _ in range(3):
            f()
    ctx.sync()
    ts = {k: [] for k in calls}
    for _ in range(repeats):  # interleaved: a drift of the machine shows in both
        for k, f in calls.items():
            ctx._chk(L.hmx_event_record(ctx.h, ev[0]))
            for _ in range(INNER):
                f()
            ctx._chk(L.hmx_event_record(ctx.h, ev[1]))
            ctx.sync()
            ms = C.c_float()
            ctx._chk(L.hmx_event_elapsed_ms(ctx.h, ev[0], ev[1], C.byref(ms)))
            ts[k].append(ms.value / INNER)
    px = NP * W * H
    for k, t in ts.items():
        med = float(np.median(t))
        print(f"{k:<11s} {med:8.3f} ms a call (min {min(t):.3f}, max {max(t):.3f}; {len(t)} repeats of {INNER} calls, HIP events)  {px / med / 1e6:6.1f} Gpx/s")
    if have_wp:
        print(f"weighted / unweighted (medians): {np.median(ts['weighted']) / np.median(ts['unweighted']):.3f}")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent", help="an older libhmx.so to time the unweighted call of, loaded through HMX_LIB_PATH")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_wp_bench.txt"))
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    a = ap.parse_args()
    if a.child:
        return child(a.repeats)
    steps = [None] + ([a.parent, None, a.parent] if a.parent else [])
    text = []
    for lib in steps:
        env = dict(os.environ)
        env.pop("HMX_LIB_PATH", None)
        if lib:
            env["HMX_LIB_PATH"] = os.path.abspath(lib)
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        text.append(f"== {'the older build (HMX_LIB_PATH)' if lib else 'this build'}\n{r.stdout}")
        print(text[-1], flush=True)
        if r.returncode != 0:  # nothing more is started on the device after a failure
            print(r.stderr[-2000:], file=sys.stderr)
            sys.exit(f"step failed with exit status {r.returncode}")
    with open(a.out, "w") as f:
        f.write("python tools/mc_wp_bench.py" + (" --parent OLDER_LIBHMX_SO" if a.parent else "") + f" --repeats {a.repeats}\n" + "".join(text))


if __name__ == "__main__":
    main()
