"""Times of the occlusion query (frr_query_pixels).  Scene (i) of tools/drawlist_times.py -- 4,096 items over 16 meshes of
12..200 triangles -- behind an occluder, a quad in front of the right part of the view; 1920 x 1080, default options.
Two probe passes over the occluder's depth: (a) the items' box proxies (scenes.box_proxy), (b) the items' own meshes.

  1. The query's tile kernel beside its yardstick: the FRR_PS_DEPTH tile kernel of the same geometry pass in the same window
     over the same depth at the PARENT commit, fragment counting enabled (it evaluates the same fragments, and resolves keys
     and writes on top).  Both are the k_raster time of frr_profile_get for the one launch, one frame at a time.  The builds
     alternate: RUNS rounds, in each one process per build (--root: the checkout whose package the process imports), each
     measuring one launch per workload after its warm-up.  The bound: the query's median is at most the parent's median
     plus the parent's own max - min -- required on (a), reported on (b).
  2. The two-pass loop on this build: clear, occluder, geometry_list(proxies), query_pixels, draw_list_if(items, counts)
     beside clear, occluder, draw_list(items); frames bracketed by device events (frr_event_record around the frame's
     commands), the same frames on the host clock (frr_clear .. frr_sync), and the fraction of items skipped.  Figures, not
     gates.

With --bench PARENT.jsonl THIS.jsonl (the JSON result lines of `python bench.py --steps 50 --warmup 5`, alternating runs) the
headline's medians and spreads are appended with the same bound.  Writes what profiles/query_times.txt holds.

  python tools/query_times.py [out.txt] --parent PARENT_CHECKOUT [--bench parent.jsonl this.jsonl]"""
import importlib.util
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else HERE
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first, see tests/conftest.py)
import numpy as np  # noqa: E402

import f_renderer_amd as fr  # noqa: E402
from f_renderer_amd import scenes  # noqa: E402
from tools.drawlist_times import configs  # noqa: E402
from tools.instanced_times import H, RUNS, W, WARM, bench_summary, fmt, frame_ms, grid_models  # noqa: E402

INFLATE = 0.002     # about a pixel's worth at 1080 rows


def box_proxy(tris):
    """scenes.box_proxy of THIS checkout (the parent's package has none; host arithmetic only)"""
    spec = importlib.util.spec_from_file_location("_scenes_here", os.path.join(HERE, "f_renderer_amd", "scenes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.box_proxy(tris, INFLATE)


def scene():
    """(renderer, the occluder's mesh, the item list, the proxy list, number of items)"""
    _, meshes, nitems, _ = configs()[0]
    models = grid_models(nitems)
    which = (np.arange(nitems) * 7 + np.arange(nitems) // len(meshes)) % len(meshes)
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
    r = fr.Renderer(W, H)
    r.set_texture(0, scenes.checker_texture(256, 16))
    r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye, texture_slot=0)
    ms = [r.upload_mesh(m, fr.VS_PHONG) for m in meshes]
    bs = [r.upload_mesh(box_proxy(m), fr.VS_PHONG) for m in meshes]
    quad = np.zeros((2, 3, 8), np.float32)   # in front of the right part of the grid, facing the camera
    c = np.array([[-0.2, -1.6, 1.0], [2.6, -1.6, 1.0], [2.6, 1.6, 1.0], [-0.2, 1.6, 1.0]], np.float32)
    quad[0, :, :3], quad[1, :, :3] = c[[0, 1, 2]], c[[0, 2, 3]]
    quad[:, :, 7] = 1.0
    occ = r.upload_mesh(quad, fr.VS_PHONG)
    items = r.upload_draw_list([ms[w] for w in which], models)
    proxies = r.upload_draw_list([bs[w] for w in which], models)
    return r, occ, items, proxies, nitems


def launch_us(r, occ, probe, query, buf, n):
    """k_raster of the ONE launch over the probe pass: the occluder is drawn and waited for outside the profile"""
    r.clear()
    r.draw(occ, fr.PS_DEPTH)
    r.sync()
    r.profile_enable(True, kernels=["k_raster"])
    r.profile_reset()
    r.geometry_list(probe)
    if query:
        r.query_pixels("item", out_ptr=buf.data_ptr(), entries=n)
    else:
        r.rasterization((0, W), (0, H), fr.PS_DEPTH)
    r.sync()
    ms, launches = r.profile_get("k_raster")
    r.profile_enable(False)
    assert launches == 1, launches
    return ms * 1e3


def frame_event_ms(r, body):
    """one frame between two device events: frr_event_record joins the ctx's streams, so the pair brackets the whole frame"""
    r.event_record(0)
    body()
    r.event_record(1)
    r.sync()
    return r.event_elapsed_ms(0, 1)


def child():
    """one build's share of a round: per workload, WARM launches and one timed one.  The parent measures the yardstick; this
    build measures the query, and the yardstick too (its tile kernel is the parent's: profiles/query_resource_usage.txt)."""
    r, occ, items, proxies, n = scene()
    r.set_count_fragments(True)
    buf = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res = {}
    has_query = hasattr(r, "query_pixels")
    for key, probe in (("a", proxies), ("b", items)):
        for query in ((False, True) if has_query else (False,)):
            for _ in range(WARM):
                launch_us(r, occ, probe, query, buf, n)
            res[key + ("_query" if query else "_yard")] = launch_us(r, occ, probe, query, buf, n)
    if has_query:
        res["skipped"] = float((buf.cpu().numpy() == 0).mean())   # (of the last query: the items' own meshes)
    r.close()
    print("RESULT " + json.dumps(res), flush=True)


def bound_line(what, p, t, unit, held=True):
    bound = np.median(p) + (max(p) - min(p))
    verdict = ("met" if np.median(t) <= bound else "NOT met") if held else ("within" if np.median(t) <= bound else f"missed by {np.median(t) - bound:.4f} {unit}") + " (reported)"
    return (f"  {what}: parent median {np.median(p):.4f} {unit} ({min(p):.4f} .. {max(p):.4f}), this median {np.median(t):.4f} {unit} "
            f"({min(t):.4f} .. {max(t):.4f}); bound = parent median + parent spread = {bound:.4f}: {verdict}")


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
    print(f"occlusion queries (frr_query_pixels); scene (i) of profiles/drawlist_times.txt behind a quad in front of the right part of the "
          f"view, {W} x {H}, default options, fragment counting enabled; probe passes: (a) the items' box proxies (inflate {INFLATE}), (b) "
          f"the items' own meshes; k_raster of frr_profile_get for the one launch, {WARM} warm-up launches, {RUNS} alternating rounds of one "
          f"process per build, median (min .. max)", file=out)
    runs = {"parent": [], "this": []}
    for _ in range(RUNS):
        for label, root in (("parent", parent), ("this", HERE)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root], capture_output=True, text=True, timeout=300, cwd=root)
            line = [x for x in p.stdout.split("\n") if x.startswith("RESULT ")]
            assert p.returncode == 0 and line, (label, p.returncode, p.stderr[-2000:])
            runs[label].append(json.loads(line[0][7:]))
            print(f"{label}: {line[0]}", file=sys.stderr, flush=True)
    print("\n1. the query's tile kernel (this build) beside the FRR_PS_DEPTH tile kernel of the same pass, window and depth at the parent "
          "commit (fragment counting enabled)", file=out)
    for key, what, held in (("a", "(a) box proxies", True), ("b", "(b) own meshes", False)):
        p = [x[key + "_yard"] for x in runs["parent"]]
        t = [x[key + "_query"] for x in runs["this"]]
        y = [x[key + "_yard"] for x in runs["this"]]
        print(bound_line(what, p, t, "us", held), file=out)
        print(f"      (the FRR_PS_DEPTH tile kernel on this build: median {np.median(y):.4f} us ({min(y):.4f} .. {max(y):.4f}))", file=out)
    print(f"  items of (b) whose own mesh counts 0 behind the occluder: {100.0 * np.median([x['skipped'] for x in runs['this']]):.1f} %", file=out)

    # 2. the two-pass loop beside drawing the whole list
    r, occ, items, proxies, n = scene()
    buf = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def whole():
        r.clear()
        r.draw(occ, fr.PS_PHONG)
        r.draw_list(items, fr.PS_PHONG)

    def loop():
        r.clear()
        r.draw(occ, fr.PS_PHONG)
        r.geometry_list(proxies)
        r.query_pixels("item", out_ptr=buf.data_ptr(), entries=n)
        r.draw_list_if(items, buf.data_ptr(), n, fr.PS_PHONG)
    whole()
    cw, dw, _ = r.readback()
    loop()
    cl, dl, _ = r.readback()
    same = bool((cw == cl).all() and (dw.view(np.uint32) == dl.view(np.uint32)).all())
    skipped = float((buf.cpu().numpy() == 0).mean())
    bodies = {"whole": whole, "loop": loop}
    for body in bodies.values():
        for _ in range(WARM):
            frame_ms(r, body)
    t = {b: [] for b in bodies}
    e = {b: [] for b in bodies}
    for _ in range(RUNS):
        for b, body in bodies.items():
            e[b].append(frame_event_ms(r, body))
        for b, body in bodies.items():
            t[b].append(frame_ms(r, body))
    print(f"\n2. the two-pass loop on this build (PS_PHONG; median of {RUNS} alternating single frames)", file=out)
    for what, v in (("between device events around the frame's commands", e), ("frr_clear .. frr_sync on the host clock", t)):
        print(f"  {what}:", file=out)
        print(f"    clear, occluder, draw_list(items)                                             {fmt(v['whole'])}", file=out)
        print(f"    clear, occluder, geometry_list(proxies), query_pixels, draw_list_if(items)    {fmt(v['loop'])}", file=out)
    print(f"    items skipped by their box proxy: {100.0 * skipped:.1f} % of {n}; the loop's frame == the whole list's frame (colour, depth): {same}", file=out)
    r.close()

    if bench:
        print("\nheadline, python bench.py --steps 50 --warmup 5, alternating runs of the parent commit and of this one:", file=out)
        res = {}
        for label, path in zip(("parent", "this"), bench):
            ms, tri = bench_summary(path)
            res[label] = ms
            print(f"  {label:6s}: {len(ms)} runs, Mtri/s median {np.median(tri):.1f} ({min(tri):.1f} .. {max(tri):.1f})", file=out)
        print(bound_line("ms_per_step", res["parent"], res["this"], "ms"), file=out)


if __name__ == "__main__":
    main()
