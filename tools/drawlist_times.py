"""Frame times of a list pass (frr_draw_list) beside the only way there was before it.  Per scene, one 1920 x 1080 frame at a
time, VS_PHONG / PS_PHONG:
  (a) list       clear + draw_list(list): one geometry pass over the items' triangles
  (b) loop       clear + for every item { set_uniforms(model=...) ; draw(mesh) }: one draw per object (phong.rs:319-359)
  (c) instanced  only for the variant of a scene whose items all name ONE mesh: clear + draw_instanced(mesh, table), beside
                 the list pass over the same objects
Each figure is a frame's time from the call of frr_clear until frr_sync returns (host clock: the loop's cost is host waits as
much as device work), the median of RUNS single frames with min .. max; the bodies alternate within one process.  Beside
them: the device time of the geometry kernels (k_geom of frr_profile_get) of the list pass and of the instanced pass.
Scenes: (i) 4,096 items over 16 distinct meshes of 12..200 triangles; (ii) 256 items over 8 distinct 4,096-triangle meshes;
(iii) three items of large, different meshes (the shape of phong.rs:319-359).
The conditions: the frames of (a) and (b) are equal byte for byte (colour, depth, ids) on every scene, and on (i) and (ii)
(a) is faster than (b) by more than the larger of the two min .. max spreads.

With --bench PARENT.jsonl THIS.jsonl (the JSON result lines of `python bench.py --steps 50 --warmup 5`, alternating runs of
the parent commit and of this one) the headline's medians and spreads are appended, with the bound: this commit's median
ms_per_step does not exceed the parent's median plus the parent's own min .. max spread.  Writes what
profiles/drawlist_times.txt holds.

  python tools/drawlist_times.py [out.txt] [--bench parent.jsonl this.jsonl]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first, see tests/conftest.py)
import numpy as np  # noqa: E402

import f_renderer_amd as fr  # noqa: E402
from f_renderer_amd import scenes  # noqa: E402
from tools.instanced_times import H, RUNS, W, WARM, bench_summary, fmt, frame_ms, geom_us, grid_models, unit  # noqa: E402

SMALL = [(3, 2), (3, 3), (4, 3), (4, 4), (5, 4), (6, 4), (6, 5), (7, 5), (8, 5), (8, 6), (9, 6), (10, 6), (10, 7), (10, 8), (10, 9), (10, 10)]
RATIOS = [(1.0, 0.4), (1.0, 0.2), (1.0, 0.6), (0.8, 0.5), (1.2, 0.3), (0.9, 0.45), (1.1, 0.15), (0.7, 0.6)]


def configs():
    small = [unit(scenes.torus(a, b)) for a, b in SMALL]
    assert len(small) == 16 and all(12 <= m.shape[0] <= 200 for m in small)
    mid = [unit(scenes.torus(64, 32, R=R, r=r)) for R, r in RATIOS]
    assert all(m.shape[0] == 4096 for m in mid)
    big = [unit(scenes.displaced_sphere(n=256)), unit(scenes.torus(256, 128)), unit(scenes.displaced_sphere(n=128, bump=0.2))]
    return (("(i) 4,096 items over 16 meshes of 12..200 triangles", small, 4096, True),
            ("(ii) 256 items over 8 meshes of 4,096 triangles", mid, 256, True),
            ("(iii) three items of large, different meshes", big, 3, False))


def main():
    argv = sys.argv[1:]
    bench = None
    if "--bench" in argv:
        k = argv.index("--bench")
        bench = argv[k + 1:k + 3]
        argv = argv[:k] + argv[k + 3:]
    out = open(argv[0], "w") if argv else sys.stdout
    print(f"a list pass beside one draw per item (and, where all items name one mesh, beside the instanced pass); {W} x {H}, VS_PHONG / "
          f"PS_PHONG, default options; one frame at a time, frr_clear .. frr_sync on the host clock, {WARM} warm-up frames each, median of "
          f"{RUNS} alternating single frames (min .. max)", file=out)
    verdicts = []
    for name, meshes, nitems, held in configs():
        models = grid_models(nitems)
        which = (np.arange(nitems) * 7 + np.arange(nitems) // len(meshes)) % len(meshes)
        eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
        r = fr.Renderer(W, H)
        r.set_texture(0, scenes.checker_texture(256, 16))
        r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye, texture_slot=0)
        ms = [r.upload_mesh(m, fr.VS_PHONG) for m in meshes]
        items = [ms[w] for w in which]
        lst = r.upload_draw_list(items, models)
        one = r.upload_draw_list([ms[0]] * nitems, models)
        table = r.upload_instances(models)
        ident = np.eye(4, dtype=np.float32).reshape(16)

        def as_list():
            r.clear()
            r.draw_list(lst, fr.PS_PHONG)

        def loop():
            r.clear()
            for mesh, mdl in zip(items, models):
                r.set_uniforms(model=mdl)
                r.draw(mesh, fr.PS_PHONG)
            r.set_uniforms(model=ident)

        def one_list():
            r.clear()
            r.draw_list(one, fr.PS_PHONG)

        def instanced():
            r.clear()
            r.draw_instanced(ms[0], table, fr.PS_PHONG)

        as_list()
        ca, da, ta = r.readback()
        sa = r.stats()
        loop()
        cl, dl, tl = r.readback()
        same = bool((ca == cl).all() and (da.view(np.uint32) == dl.view(np.uint32)).all() and (ta == tl).all())
        one_list()
        co, do, to = r.readback()
        instanced()
        ci, di, ti = r.readback()
        same_one = bool((co == ci).all() and (do.view(np.uint32) == di.view(np.uint32)).all() and (to == ti).all())
        bodies = {"list": as_list, "loop": loop, "one_list": one_list, "instanced": instanced}
        for body in bodies.values():
            for _ in range(WARM):
                frame_ms(r, body)
        runs = {k: [] for k in bodies}
        for _ in range(RUNS):
            for k, body in bodies.items():
                runs[k].append(frame_ms(r, body))
        gl, nl = geom_us(r, as_list)
        go, no = geom_us(r, one_list)
        gi, ni = geom_us(r, instanced)
        print(f"\n{name}: {sa['tris_in']} inputs; tris_setup {sa['tris_setup']}, covered fragments {sa['frag_covered']}, drawn share "
              f"{float((ta != 0xFFFFFFFF).mean()):.3f}; list frame == loop frame (colour, depth, ids): {same}", file=out)
        print(f"  (a) list       {fmt(runs['list'])}", file=out)
        print(f"  (b) loop       {fmt(runs['loop'])}", file=out)
        a, b = runs["list"], runs["loop"]
        margin, spread = np.median(b) - np.median(a), max(max(a) - min(a), max(b) - min(b))
        ok = bool(margin > spread)
        verdicts.append(same and (ok or not held))
        print(f"  loop - list = {margin:.3f} ms, larger min .. max spread {spread:.3f} ms: condition {'met' if ok else 'NOT met'}"
              f"{'' if held else ' (reported, not held on this scene)'} (loop / list = {np.median(b) / np.median(a):.1f})", file=out)
        print(f"  k_geom per frame, list: {gl:9.1f} us ({nl} launches)", file=out)
        print(f"  the variant whose {nitems} items all name mesh 0 ({meshes[0].shape[0]} triangles); list frame == instanced frame: {same_one}", file=out)
        print(f"    list       {fmt(runs['one_list'])}   k_geom {go:9.1f} us ({no} launches)", file=out)
        print(f"    (c) instanced  {fmt(runs['instanced'])}   k_geom {gi:9.1f} us ({ni} launches): list / instanced k_geom = {go / gi:.2f}", file=out)
        verdicts.append(same_one)
        r.close()
    print(f"\nconditions (equal frames everywhere; (a) faster than (b) beyond the spread on (i) and (ii)): {'met' if all(verdicts) else 'NOT met'}", file=out)
    print("the wave-uniform search of the item (one search per wave, per-lane only where a wave spans items) is the only build: no per-lane-only "
          "build was made to set beside it", file=out)
    if bench:
        print("\nheadline, python bench.py --steps 50 --warmup 5 (the non-list path), alternating runs of the parent commit and of this one:", file=out)
        res = {}
        for label, path in zip(("parent", "this  "), bench):
            ms, tri = bench_summary(path)
            res[label] = ms
            print(f"  {label}: {len(ms)} runs, ms_per_step median {np.median(ms):.4f} ({min(ms):.4f} .. {max(ms):.4f}), Mtri/s median {np.median(tri):.1f} "
                  f"({min(tri):.1f} .. {max(tri):.1f})", file=out)
        p, t = res["parent"], res["this  "]
        bound = np.median(p) + (max(p) - min(p))
        print(f"  bound: parent median + parent min .. max spread = {bound:.4f} ms per step; this median {np.median(t):.4f}: "
              f"{'met' if np.median(t) <= bound else 'NOT met'}", file=out)


if __name__ == "__main__":
    main()
