"""Times of the box query (frr_drawlist_bounds / frr_query_boxes) beside the proxy path it replaces.  The scene of
tools/query_times.py: 4,096 items over 16 meshes of 12..200 triangles behind a quad in front of the right part of the view;
1920 x 1080, default options.  Its protocol: WARM warm-ups, RUNS alternating rounds, median (min .. max).

  1. Device time (frr_profile_get, event pairs around the launches) of one frr_query_boxes -- the pyramid of the window's depth
     and the test of every item -- and of one frr_drawlist_bounds; beside them, in the same session on the same build, the
     proxy path's kernels for one query: the geometry pass of the box proxies, its binning, the query's tile kernel and prep.
  2. Three frames between device events and on the host clock: draw everything; the proxy loop (clear, occluder,
     geometry_list(proxies), query_pixels, draw_list_if); the box loop (clear, occluder, query_boxes, draw_list_if).
  3. The share of the items each test skips, and whether each loop's colour and depth equal the whole list's.

With --bench PARENT.jsonl THIS.jsonl (the JSON result lines of `python bench.py --steps 50 --warmup 5`, alternating runs) the
headline's medians and spreads are appended with the project's bound.  Writes what profiles/boxes_times.txt holds.

  python tools/boxes_times.py [out.txt] [--bench parent.jsonl this.jsonl]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (first, see tests/conftest.py)
import numpy as np  # noqa: E402

import f_renderer_amd as fr  # noqa: E402
from tools.instanced_times import H, RUNS, W, WARM, bench_summary, fmt, frame_ms  # noqa: E402
from tools.query_times import bound_line, frame_event_ms, scene  # noqa: E402

PROXY_KERNELS = ["k_geom", "k_geom_scan", "k_bin_count", "k_tile_scan", "k_bin_fill", "k_bin_seg", "k_raster", "k_visible"]


def us(v):
    return f"{np.median(v):9.2f} us  ({min(v):9.2f} .. {max(v):9.2f})"


def device_us(r, kernels, body, prepare):
    """device time of `kernels` over one `body`, whose frame `prepare` has drawn and waited for outside the profile"""
    prepare()
    r.sync()
    r.profile_enable(True, kernels=kernels)
    r.profile_reset()
    body()
    r.sync()
    total = sum(r.profile_get(k)[0] for k in kernels) * 1e3
    r.profile_enable(False)
    return total


def main():
    argv = sys.argv[1:]
    bench = None
    if "--bench" in argv:
        k = argv.index("--bench")
        bench = argv[k + 1:k + 3]
        argv = argv[:k] + argv[k + 3:]
    out = open(argv[0], "w") if argv else sys.stdout
    r, occ, items, proxies, n = scene()
    buf = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    print(f"box queries (frr_drawlist_bounds, frr_query_boxes); the scene of profiles/query_times.txt: {n} items over 16 meshes behind a quad "
          f"in front of the right part of the view, {W} x {H}, default options; {WARM} warm-ups, {RUNS} alternating rounds, median (min .. max)", file=out)

    def occluder():
        r.clear()
        r.draw(occ, fr.PS_DEPTH)

    def boxes():
        r.query_boxes(items, out_ptr=buf.data_ptr(), entries=n)

    def proxy():
        r.geometry_list(proxies)
        r.query_pixels("item", out_ptr=buf.data_ptr(), entries=n)

    def bounds():
        r.list_bounds(items)
    bounds()
    t_bounds, d = [], {"boxes": [], "proxy": [], "bounds": []}
    for k in range(WARM + RUNS):
        t0 = time.perf_counter()
        bounds()
        tb = (time.perf_counter() - t0) * 1e3
        row = {"bounds": device_us(r, ["k_boxes"], bounds, occluder), "boxes": device_us(r, ["k_boxes"], boxes, occluder),
               "proxy": device_us(r, PROXY_KERNELS, proxy, occluder)}
        if k >= WARM:
            t_bounds.append(tb)
            for key, v in row.items():
                d[key].append(v)
    print("\n1. device time of the kernels of one command (frr_profile_get), the occluder drawn and waited for outside the profile", file=out)
    print(f"  frr_query_boxes (k_boxes: depth pyramid + the test of {n} items)                          {us(d['boxes'])}", file=out)
    print(f"  the proxy path: geometry_list(proxies) + query_pixels ({' + '.join(PROXY_KERNELS)})\n"
          f"                                                                                           {us(d['proxy'])}", file=out)
    print(f"  frr_drawlist_bounds, once per list (k_boxes: 16 reductions + the per-item table)          {us(d['bounds'])}", file=out)
    print(f"  frr_drawlist_bounds on the host clock (a synchronisation point, four small copies)        {fmt(t_bounds)}", file=out)

    def whole():
        r.clear()
        r.draw(occ, fr.PS_PHONG)
        r.draw_list(items, fr.PS_PHONG)

    def proxy_loop():
        r.clear()
        r.draw(occ, fr.PS_PHONG)
        r.geometry_list(proxies)
        r.query_pixels("item", out_ptr=buf.data_ptr(), entries=n)
        r.draw_list_if(items, buf.data_ptr(), n, fr.PS_PHONG)

    def box_loop():
        r.clear()
        r.draw(occ, fr.PS_PHONG)
        r.query_boxes(items, out_ptr=buf.data_ptr(), entries=n)
        r.draw_list_if(items, buf.data_ptr(), n, fr.PS_PHONG)
    whole()
    cw, dw, _ = r.readback()
    same, skipped = {}, {}
    for name, body in (("proxy", proxy_loop), ("box", box_loop)):
        body()
        c, dd, _ = r.readback()
        same[name] = bool((cw == c).all() and (dw.view(np.uint32) == dd.view(np.uint32)).all())
        skipped[name] = float((buf.cpu().numpy() == 0).mean())
    bodies = {"whole": whole, "proxy": proxy_loop, "box": box_loop}
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
    print(f"\n2. three frames (PS_PHONG; {RUNS} alternating single frames)", file=out)
    for what, v in (("between device events around the frame's commands", e), ("frr_clear .. frr_sync on the host clock", t)):
        print(f"  {what}:", file=out)
        print(f"    clear, occluder, draw_list(items)                                             {fmt(v['whole'])}", file=out)
        print(f"    clear, occluder, geometry_list(proxies), query_pixels, draw_list_if(items)    {fmt(v['proxy'])}", file=out)
        print(f"    clear, occluder, query_boxes(items), draw_list_if(items)                      {fmt(v['box'])}", file=out)
    print(f"\n3. items skipped: by their box proxy's query {100.0 * skipped['proxy']:.1f} %, by the box query {100.0 * skipped['box']:.1f} % of {n}", file=out)
    print(f"4. the loop's frame == the whole list's frame (colour, depth): proxy loop {same['proxy']}, box loop {same['box']}", file=out)
    spread = max(max(e[b]) - min(e[b]) for b in bodies)
    print(f"   the box loop against the better of the other two, between device events: {np.median(e['box']):.3f} ms vs "
          f"{min(np.median(e['whole']), np.median(e['proxy'])):.3f} ms; the rounds' largest spread: {spread:.3f} ms", file=out)
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
