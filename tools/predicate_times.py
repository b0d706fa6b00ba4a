"""Frame times around predicated list passes (frr_draw_list_if).  Scenes (i) and (ii) of tools/drawlist_times.py -- 4,096
items over 16 meshes of 12..200 triangles; 256 items over 8 meshes of 4,096 triangles -- with its protocol: 1920 x 1080,
VS_PHONG / PS_PHONG, default options, one frame at a time from the call of frr_clear until frr_sync returns on the host
clock, 2 warm-up frames, the median of 7 alternating single frames with min .. max.

  1. The unpredicated list path on this build beside the parent commit's: frr_draw_list frame time and k_geom of
     frr_profile_get.  The two builds alternate: seven rounds, in each one process per build (--root: the checkout whose
     package the process imports), each measuring one frame per scene after its warm-up.  The bound is the one
     profiles/drawlist_times.txt uses: this build's median is at most the parent's median plus the parent's own
     min .. max spread.
  2. What a predicate buys, on this build: frr_draw_list_if under seeded random masks that keep 100 %, 50 %, 10 % and 0 % of
     the items, and a 50 % mask that keeps whole runs of 64 consecutive items, beside frr_draw_list of a list uploaded
     with the kept items only -- the alternative a caller has today, whose frr_drawlist_upload is timed separately on the
     host clock.  Frame time, and k_geom, k_bin_seg and k_raster per frame.  The 100 % predicated frame beside the
     unpredicated one is the cost of the keep table and of the verification inside the call.

With --bench PARENT.jsonl THIS.jsonl (the JSON result lines of `python bench.py --steps 50 --warmup 5`, five alternating runs
each) the headline's medians and spreads are appended with the same bound.  Writes what profiles/predicate_times.txt holds.

  python tools/predicate_times.py [out.txt] --parent PARENT_CHECKOUT [--bench parent.jsonl this.jsonl]"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else HERE
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first, see tests/conftest.py)
import numpy as np  # noqa: E402

import f_renderer_amd as fr  # noqa: E402
from f_renderer_amd import scenes  # noqa: E402
from tools.drawlist_times import configs  # noqa: E402
from tools.instanced_times import H, RUNS, W, WARM, bench_summary, fmt, frame_ms, grid_models  # noqa: E402

KERNELS = ["k_geom", "k_bin_seg", "k_raster"]
MASKS = [("random 100 %", 1.0, 0), ("random 50 %", 0.5, 0), ("random 10 %", 0.1, 0), ("random 0 %", 0.0, 0), ("runs of 64, 50 %", 0.5, 64)]


def scene(k):
    """(name, renderer, the meshes of its items, models) of scene k of tools/drawlist_times.py"""
    name, meshes, nitems, _ = configs()[k]
    models = grid_models(nitems)
    which = (np.arange(nitems) * 7 + np.arange(nitems) // len(meshes)) % len(meshes)
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
    r = fr.Renderer(W, H)
    r.set_texture(0, scenes.checker_texture(256, 16))
    r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye, texture_slot=0)
    ms = [r.upload_mesh(m, fr.VS_PHONG) for m in meshes]
    return name, r, [ms[w] for w in which], models


def kernels_us(r, body, frames=5):
    """device time per frame of KERNELS (frr_profile_get: event pairs around every launch)"""
    r.profile_enable(True, kernels=KERNELS)
    r.profile_reset()
    for _ in range(frames):
        body()
        r.sync()
    out = [r.profile_get(k)[0] * 1e3 / frames for k in KERNELS]
    r.profile_enable(False)
    return out


def child():
    """one build's share of a round: per scene, WARM frames, one timed frr_draw_list frame, k_geom per frame"""
    res = []
    for k in (0, 1):
        _, r, items, models = scene(k)
        lst = r.upload_draw_list(items, models)

        def body():
            r.clear()
            r.draw_list(lst, fr.PS_PHONG)
        for _ in range(WARM):
            frame_ms(r, body)
        ms = frame_ms(r, body)
        res.append({"ms": ms, "k_geom_us": kernels_us(r, body)[0]})
        r.close()
    print("RESULT " + json.dumps(res), flush=True)


def mask_of(n, share, run, seed):
    rng = np.random.default_rng(seed)
    if run:
        m = np.repeat(rng.permutation(np.arange((n + run - 1) // run) % 2 == 0), run)[:n]
    else:
        m = np.zeros(n, bool)
        m[rng.permutation(n)[:int(round(share * n))]] = True
    return m


def bound_line(what, p, t, unit):
    bound = np.median(p) + (max(p) - min(p))
    return (f"  {what}: parent median {np.median(p):.4f} {unit} ({min(p):.4f} .. {max(p):.4f}), this median {np.median(t):.4f} {unit} "
            f"({min(t):.4f} .. {max(t):.4f}); bound = parent median + parent spread = {bound:.4f}: {'met' if np.median(t) <= bound else 'NOT met'}")


def main():
    argv = sys.argv[1:]
    if "--child" in argv:
        return child()
    bench = None
    if "--bench" in argv:
        k = argv.index("--bench")
        bench = argv[k + 1:k + 3]
        argv = argv[:k] + argv[k + 3:]
    k = argv.index("--parent")
    parent = os.path.abspath(argv[k + 1])
    argv = argv[:k] + argv[k + 2:]
    out = open(argv[0], "w") if argv else sys.stdout
    print(f"predicated list passes (frr_draw_list_if); scenes (i) and (ii) of profiles/drawlist_times.txt, {W} x {H}, VS_PHONG / PS_PHONG, default "
          f"options; one frame at a time, frr_clear .. frr_sync on the host clock, {WARM} warm-up frames, median of {RUNS} alternating single "
          f"frames (min .. max); kernel times: frr_profile_get per frame", file=out)
    names = [configs()[k][0] for k in (0, 1)]

    # 1. the unpredicated list path, this build beside the parent commit's
    print("\n1. the unpredicated list path (frr_draw_list): this build beside the parent commit built from a clean checkout; the builds "
          f"alternate, {RUNS} rounds of one process per build", file=out)
    runs = {"parent": [], "this": []}
    for _ in range(RUNS):
        for label, root in (("parent", parent), ("this", HERE)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root], capture_output=True, text=True, timeout=300, cwd=root)
            line = [x for x in p.stdout.split("\n") if x.startswith("RESULT ")]
            assert p.returncode == 0 and line, (label, p.returncode, p.stderr[-2000:])
            runs[label].append(json.loads(line[0][7:]))
            print(f"round {len(runs['this']) + (label == 'parent')} {label}: {line[0]}", file=sys.stderr, flush=True)
    verdicts = []
    for k in (0, 1):
        print(f"\n{names[k]}", file=out)
        for key, unit in (("ms", "ms"), ("k_geom_us", "us")):
            p, t = [x[k][key] for x in runs["parent"]], [x[k][key] for x in runs["this"]]
            text = bound_line("frame" if key == "ms" else "k_geom per frame", p, t, unit)
            verdicts.append(text.endswith(": met"))
            print(text, file=out)
    print(f"\nbound on the unpredicated list path (frame time and k_geom, both scenes): {'met' if all(verdicts) else 'NOT met'}", file=out)

    # 2. what a predicate buys
    print("\n2. frr_draw_list_if beside frr_draw_list of a list uploaded with the kept items only (its frr_drawlist_upload timed on the host "
          "clock, median of 7); this build", file=out)
    for k in (0, 1):
        name, r, items, models = scene(k)
        n = len(items)
        lst = r.upload_draw_list(items, models)

        def plain():
            r.clear()
            r.draw_list(lst, fr.PS_PHONG)
        print(f"\n{name}", file=out)
        rows = []
        for label, share, run in MASKS:
            m = mask_of(n, share, run, 20261020 + k)
            dev = torch.from_numpy(m.astype(np.int32)).to("cuda")
            torch.cuda.synchronize()
            idx = np.nonzero(m)[0]
            ups = []
            for j in range(RUNS):
                t0 = time.perf_counter()
                sub = r.upload_draw_list([items[i] for i in idx], models[idx])
                ups.append((time.perf_counter() - t0) * 1e3)
                if j + 1 < RUNS:
                    r.free_draw_list(sub)

            def pred():
                r.clear()
                r.draw_list_if(lst, dev.data_ptr(), n, fr.PS_PHONG)

            def kept_only():
                r.clear()
                r.draw_list(sub, fr.PS_PHONG)
            pred()
            cp, dp, _ = r.readback()
            sp = r.stats()
            kept_only()
            cs, ds, _ = r.readback()
            same = bool((cp == cs).all() and (dp.view(np.uint32) == ds.view(np.uint32)).all())
            bodies = {"pred": pred, "sub": kept_only, "plain": plain}
            for body in bodies.values():
                for _ in range(WARM):
                    frame_ms(r, body)
            t = {b: [] for b in bodies}
            for _ in range(RUNS):
                for b, body in bodies.items():
                    t[b].append(frame_ms(r, body))
            ku = {b: kernels_us(r, body) for b, body in bodies.items()}
            rows.append((label, t, ku))
            print(f"{name}: mask {label} done", file=sys.stderr, flush=True)
            print(f"  mask {label}: {int(m.sum())} of {n} items kept, tris_setup {sp['tris_setup']}; predicated frame == kept-items frame (colour, depth): {same}", file=out)
            for b, what in (("pred", "frr_draw_list_if          "), ("sub", "frr_draw_list, kept items ")):
                print(f"    {what} {fmt(t[b])}   " + "  ".join(f"{kn} {v:7.1f} us" for kn, v in zip(KERNELS, ku[b])), file=out)
            print(f"    frr_drawlist_upload of the kept items (host clock): {np.median(ups):.3f} ms ({min(ups):.3f} .. {max(ups):.3f})", file=out)
            r.free_draw_list(sub)
        label, t, ku = rows[0]
        print("  the 100 % predicated frame beside the unpredicated one (keep table + verification inside the call):", file=out)
        print(f"    frr_draw_list_if           {fmt(t['pred'])}   " + "  ".join(f"{kn} {v:7.1f} us" for kn, v in zip(KERNELS, ku["pred"])), file=out)
        print(f"    frr_draw_list              {fmt(t['plain'])}   " + "  ".join(f"{kn} {v:7.1f} us" for kn, v in zip(KERNELS, ku["plain"])), file=out)
        print(f"    difference of the medians: {np.median(t['pred']) - np.median(t['plain']):+.3f} ms (reported, not held to a bound)", file=out)
        r.close()

    if bench:
        print("\nheadline, python bench.py --steps 50 --warmup 5 (the non-list path), alternating runs of the parent commit and of this one:", file=out)
        res = {}
        for label, path in zip(("parent", "this"), bench):
            ms, tri = bench_summary(path)
            res[label] = ms
            print(f"  {label:6s}: {len(ms)} runs, Mtri/s median {np.median(tri):.1f} ({min(tri):.1f} .. {max(tri):.1f})", file=out)
        print(bound_line("ms_per_step", res["parent"], res["this"], "ms"), file=out)


if __name__ == "__main__":
    main()
