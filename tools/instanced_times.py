"""Frame times of an instanced pass (frr_draw_instanced) beside the two ways there were before it.  Per scene, one 1920 x 1080
frame at a time, VS_PHONG / PS_PHONG:
  (a) instanced  clear + draw_instanced(mesh, table): one geometry pass over the (instance, triangle) pairs
  (b) loop       clear + for every matrix { set_uniforms(model=...) ; draw(mesh) }: one draw per object (phong.rs:319-331)
  (c) expanded   clear + draw(one mesh of ninst * ntris triangles with the transforms baked in): ninst times the memory, and
                 other bits ((proj*view*model)*p is not (proj*view)*(model*p) in f32) -- for the time only
Each figure is a frame's time from the call of frr_clear until frr_sync returns (host clock: the loop's cost is host waits as
much as device work), the median of RUNS single frames with min .. max; the three alternate within one process.  Beside
them: the device time of the geometry kernels (k_geom of frr_profile_get) of (a) and (c).
Scenes: 4,096 instances of the 12-triangle cube; 256 instances of a 4,096-triangle torus; 8 instances of a 131,072-triangle
sphere.
The condition: on every scene (a) is faster than (b) by more than the larger of the two min .. max spreads.

With --bench PARENT.jsonl THIS.jsonl (the JSON result lines of `python bench.py --steps 50 --warmup 5`, several runs each, of
the parent commit and of this one) the headline's medians and spreads are appended.  Writes what
profiles/instanced_times.txt holds.

  python tools/instanced_times.py [out.txt] [--bench parent.jsonl this.jsonl]"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first, see tests/conftest.py)
import numpy as np  # noqa: E402

import f_renderer_amd as fr  # noqa: E402
from f_renderer_amd import scenes  # noqa: E402

W, H = 1920, 1080
WARM, RUNS = 2, 7


def grid_models(k, extent=(3.6, 2.0), fill=0.8):
    """k translations on a grid across the view, scaled so that neighbours do not touch: [k, 16] column-major"""
    cols = max(1, int(math.ceil(math.sqrt(k * extent[0] / extent[1]))))
    rows = (k + cols - 1) // cols
    s = np.float32(fill * min(extent[0] / cols, extent[1] / rows))
    m = np.tile(np.eye(4, dtype=np.float32).reshape(16), (k, 1))
    i = np.arange(k)
    m[:, 0] = m[:, 5] = m[:, 10] = s
    m[:, 12] = ((i % cols + 0.5) / cols - 0.5) * extent[0]
    m[:, 13] = ((i // cols + 0.5) / rows - 0.5) * extent[1]
    m[:, 14] = -0.2 * (i % 3)
    return m


def unit(mesh):
    """the mesh scaled into the unit cube around the origin"""
    p = mesh[..., :3]
    c, e = (p.max((0, 1)) + p.min((0, 1))) / 2, (p.max((0, 1)) - p.min((0, 1))).max()
    out = mesh.copy()
    out[..., :3] = (p - c) / e
    return out.astype(np.float32)


def expanded(mesh, models):
    """one mesh with every instance's transform applied to the positions on the host"""
    out = np.empty((models.shape[0],) + mesh.shape, np.float32)
    out[...] = mesh
    for i, m in enumerate(models):
        c = m.reshape(4, 4)                                 # [column][row]
        out[i, ..., :3] = mesh[..., 0:1] * c[0, :3] + mesh[..., 1:2] * c[1, :3] + mesh[..., 2:3] * c[2, :3] + c[3, :3]
    return out.reshape(-1, 3, mesh.shape[2])


def frame_ms(r, body):
    t0 = time.perf_counter()
    body()
    r.sync()
    return (time.perf_counter() - t0) * 1e3


def geom_us(r, body, frames=5):
    """device time of the geometry kernels per frame (frr_profile_get: event pairs around every k_geom launch)"""
    r.profile_enable(True, kernels=["k_geom"])
    r.profile_reset()
    for _ in range(frames):
        body()
        r.sync()
    ms, n = r.profile_get("k_geom")
    r.profile_enable(False)
    return ms * 1e3 / frames, n // frames


def fmt(v):
    return f"{np.median(v):10.3f} ms  ({min(v):10.3f} .. {max(v):10.3f})"


def bench_summary(path):
    vals = [json.loads(line) for line in open(path) if line.strip().startswith("{")]
    ms = [v["ms_per_step"] for v in vals]
    tri = [v["value"] for v in vals]
    return ms, tri


def main():
    argv = sys.argv[1:]
    bench = None
    if "--bench" in argv:
        k = argv.index("--bench")
        bench = argv[k + 1:k + 3]
        argv = argv[:k] + argv[k + 3:]
    out = open(argv[0], "w") if argv else sys.stdout
    from f_renderer_amd.assets import Model
    cv, cf = Model(os.path.join(ROOT, "tests", "golden", "cube.obj")).indexed_inputs()
    configs = (("4,096 x 12-triangle cube", unit(cv[cf.astype(np.int64)]), 4096),
               ("256 x 4,096-triangle torus", unit(scenes.torus(64, 32)), 256),
               ("8 x 131,072-triangle sphere", unit(scenes.displaced_sphere(n=256)), 8))
    print(f"an instanced pass beside one draw per object and beside one draw of the expanded mesh; {W} x {H}, VS_PHONG / PS_PHONG, default "
          f"options; one frame at a time, frr_clear .. frr_sync on the host clock, {WARM} warm-up frames each, median of {RUNS} alternating "
          f"single frames (min .. max)", file=out)
    verdicts = []
    for name, mesh, ninst in configs:
        models = grid_models(ninst)
        eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
        r = fr.Renderer(W, H)
        r.set_texture(0, scenes.checker_texture(256, 16))
        r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye, texture_slot=0)
        m = r.upload_mesh(mesh, fr.VS_PHONG)
        big = r.upload_mesh(expanded(mesh, models), fr.VS_PHONG)
        table = r.upload_instances(models)
        ident = np.eye(4, dtype=np.float32).reshape(16)

        def instanced():
            r.clear()
            r.draw_instanced(m, table, fr.PS_PHONG)

        def loop():
            r.clear()
            for mdl in models:
                r.set_uniforms(model=mdl)
                r.draw(m, fr.PS_PHONG)
            r.set_uniforms(model=ident)

        def baked():
            r.clear()
            r.draw(big, fr.PS_PHONG)

        instanced()
        ci, di, ti = r.readback()
        si = r.stats()
        loop()
        cl, dl, tl = r.readback()
        same = bool((ci == cl).all() and (di.view(np.uint32) == dl.view(np.uint32)).all() and (ti == tl).all())
        bodies = {"instanced": instanced, "loop": loop, "expanded": baked}
        for body in bodies.values():
            for _ in range(WARM):
                frame_ms(r, body)
        runs = {k: [] for k in bodies}
        for _ in range(RUNS):
            for k, body in bodies.items():
                runs[k].append(frame_ms(r, body))
        gi, ni = geom_us(r, instanced)
        ge, ne = geom_us(r, baked)
        print(f"\n{name}: {ninst} instances x {mesh.shape[0]} triangles = {ninst * mesh.shape[0]} inputs; tris_setup {si['tris_setup']}, covered fragments "
              f"{si['frag_covered']}, drawn share {float((ti != 0xFFFFFFFF).mean()):.3f}; instanced frame == loop frame (colour, depth, ids): {same}", file=out)
        print(f"  (a) instanced  {fmt(runs['instanced'])}", file=out)
        print(f"  (b) loop       {fmt(runs['loop'])}", file=out)
        print(f"  (c) expanded   {fmt(runs['expanded'])}", file=out)
        a, b = runs["instanced"], runs["loop"]
        margin, spread = np.median(b) - np.median(a), max(max(a) - min(a), max(b) - min(b))
        ok = bool(margin > spread)
        verdicts.append(ok and same)
        print(f"  loop - instanced = {margin:.3f} ms, larger min .. max spread {spread:.3f} ms: condition {'met' if ok else 'NOT met'} "
              f"(loop / instanced = {np.median(b) / np.median(a):.1f})", file=out)
        print(f"  k_geom per frame: instanced {gi:9.1f} us ({ni} launch), expanded {ge:9.1f} us ({ne} launch): ratio {gi / ge:.2f}", file=out)
        r.close()
    print(f"\ncondition on every scene: {'met' if all(verdicts) else 'NOT met'}", file=out)
    if bench:
        print("\nheadline, python bench.py --steps 50 --warmup 5 (the non-instanced path), runs of the parent commit and of this one:", file=out)
        res = {}
        for label, path in zip(("parent", "this  "), bench):
            ms, tri = bench_summary(path)
            res[label] = ms
            print(f"  {label}: {len(ms)} runs, ms_per_step median {np.median(ms):.4f} ({min(ms):.4f} .. {max(ms):.4f}), Mtri/s median {np.median(tri):.1f} "
                  f"({min(tri):.1f} .. {max(tri):.1f})", file=out)
        p, t = res["parent"], res["this  "]
        d, s = np.median(t) - np.median(p), max(max(p) - min(p), max(t) - min(t))
        print(f"  this - parent = {d:+.4f} ms per step, larger min .. max spread {s:.4f} ms: {'unchanged within the spread' if abs(d) <= s else 'CHANGED beyond the spread'}", file=out)


if __name__ == "__main__":
    main()
