"""Times of the visible-pixel count (frr_visible_pixels) beside the only way there was before it, at 1920 x 1080:
  per item      scene (i) of tools/drawlist_times.py: 4,096 items over 16 meshes of 12..200 triangles, one list pass
  per triangle  the 1M-triangle headline scene of bench.py (depth-only), one plain draw
Per scene the frame is drawn once, and then, alternating within one process:
  (a) count     the count command into a device buffer + frr_sync
  (b) readback  what there was: frr_readback of the ids + the NumPy search of each id's item and np.bincount (per triangle:
                np.bincount of the ids)
Host clock, WARM warm-up rounds, the median of RUNS alternating rounds with min .. max; beside them the device time of
k_visible from frr_profile_get (its zeroing / boundary launch included) and the time 4 bytes per window entry take at the
HBM rate.  The conditions: equal counts everywhere, and (a) below (b) by more than the larger of the two min .. max spreads.

With --bench PARENT.jsonl THIS.jsonl (the JSON result lines of `python bench.py --steps 50 --warmup 5`, alternating runs of
the parent commit and of this one) the headline's medians and spreads are appended, with the bound: this commit's median
ms_per_step does not exceed the parent's median plus the parent's own min .. max spread.  Writes what
profiles/visible_times.txt holds.

  python tools/visible_times.py [out.txt] [--bench parent.jsonl this.jsonl]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first, see tests/conftest.py)
import numpy as np  # noqa: E402

import f_renderer_amd as fr  # noqa: E402
from f_renderer_amd import scenes  # noqa: E402
from tools.drawlist_times import configs  # noqa: E402
from tools.instanced_times import H, RUNS, W, WARM, bench_summary, fmt, grid_models  # noqa: E402

HBM_GBS = 8000.0    # MI355X: 8 TB/s peak


def ms_of(body):
    t0 = time.perf_counter()
    out = body()
    return (time.perf_counter() - t0) * 1e3, out


def measure(out, r, name, unit, n, numpy_side):
    """n: the units; numpy_side(ids) -> the counts as the parent commit's caller computes them"""
    buf = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def count():
        r.visible_pixels(unit, out_ptr=buf.data_ptr(), entries=n)
        r.sync()

    def readback():
        return numpy_side(r.readback(False, False, True)[2])

    for _ in range(WARM):
        count()
        readback()
    ta, tb, want = [], [], None
    for _ in range(RUNS):
        ta.append(ms_of(count)[0])
        t, want = ms_of(readback)
        tb.append(t)
    got = buf.cpu().numpy().view(np.uint32)
    same = bool((got == want).all())
    r.profile_enable(True, kernels=["k_visible"])
    r.profile_reset()
    for _ in range(5):
        count()
    kms, kn = r.profile_get("k_visible")
    r.profile_enable(False)
    margin, spread = np.median(tb) - np.median(ta), max(max(ta) - min(ta), max(tb) - min(tb))
    ok = bool(margin > spread)
    path = "LDS histogram" if n <= fr.VISIBLE_LDS_BINS else "global adds"
    print(f"\n{name}: {n} units ({path}), {int((want > 0).sum())} of them own a pixel, {int(want.sum())} entries drawn of {W * H}; "
          f"count == readback + NumPy: {same}", file=out)
    print(f"  (a) count + sync        {fmt(ta)}", file=out)
    print(f"  (b) readback + NumPy    {fmt(tb)}", file=out)
    print(f"  (b) - (a) = {margin:.3f} ms, larger min .. max spread {spread:.3f} ms: condition {'met' if ok else 'NOT met'} ((b) / (a) = {np.median(tb) / np.median(ta):.1f})", file=out)
    print(f"  k_visible per command: {kms * 1e3 / max(kn, 1):9.1f} us ({kn} launches bracketed); {W * H * 4 / 1e6:.1f} MB of ids at {HBM_GBS / 1e3:.0f} TB/s: "
          f"{W * H * 4 / HBM_GBS / 1e3:.1f} us", file=out)
    return same and ok


def main():
    argv = sys.argv[1:]
    bench = None
    if "--bench" in argv:
        k = argv.index("--bench")
        bench = argv[k + 1:k + 3]
        argv = argv[:k] + argv[k + 3:]
    out = open(argv[0], "w") if argv else sys.stdout
    print(f"the visible-pixel count on the device beside a read-back of the ids and a NumPy histogram; {W} x {H}, default options; host clock, "
          f"{WARM} warm-up rounds, median of {RUNS} alternating rounds (min .. max)", file=out)
    verdicts = []
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)

    # per item: scene (i) of tools/drawlist_times.py
    name, meshes, nitems, _ = configs()[0]
    models = grid_models(nitems)
    which = (np.arange(nitems) * 7 + np.arange(nitems) // len(meshes)) % len(meshes)
    r = fr.Renderer(W, H)
    r.set_texture(0, scenes.checker_texture(256, 16))
    r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye, texture_slot=0)
    ms = [r.upload_mesh(m, fr.VS_PHONG) for m in meshes]
    lst = r.upload_draw_list([ms[w] for w in which], models)
    r.clear()
    r.draw_list(lst, fr.PS_PHONG)
    first, count = r.item_ranges()
    ends = (first.astype(np.int64) + count)

    def per_item(ids):
        v = ids[ids != 0xFFFFFFFF].astype(np.int64)
        return np.bincount(np.searchsorted(ends, v, side="right"), minlength=nitems)[:nitems].astype(np.uint32)

    verdicts.append(measure(out, r, "per item, " + name, "item", nitems, per_item))
    r.close()

    # per triangle: the headline scene
    cfg = scenes.build_config("headline")
    r = fr.Renderer(W, H)
    r.set_uniforms(flat_color=cfg["flat_color"])
    mesh = r.upload_mesh(cfg["mesh"], getattr(fr, "VS_" + cfg["vs"]))
    r.clear()
    r.draw(mesh, getattr(fr, "PS_" + cfg["ps"]))
    T = int(r.stats()["tris_setup"])

    def per_triangle(ids):
        return np.bincount(ids[ids != 0xFFFFFFFF], minlength=T)[:T].astype(np.uint32)

    verdicts.append(measure(out, r, f"per triangle, the headline scene ({cfg['mesh'].shape[0]} inputs)", "triangle", T, per_triangle))
    r.close()
    print(f"\nconditions (equal counts everywhere; (a) below (b) beyond the spread): {'met' if all(verdicts) else 'NOT met'}", file=out)
    if bench:
        print("\nheadline, python bench.py --steps 50 --warmup 5 (the path that does not count), alternating runs of the parent commit and of this one:", file=out)
        res = {}
        for label, path in zip(("parent", "this  "), bench):
            ms_, tri = bench_summary(path)
            res[label] = ms_
            print(f"  {label}: {len(ms_)} runs, ms_per_step median {np.median(ms_):.4f} ({min(ms_):.4f} .. {max(ms_):.4f}), Mtri/s median {np.median(tri):.1f} "
                  f"({min(tri):.1f} .. {max(tri):.1f})", file=out)
        p, t = res["parent"], res["this  "]
        bound = np.median(p) + (max(p) - min(p))
        print(f"  bound: parent median + parent min .. max spread = {bound:.4f} ms per step; this median {np.median(t):.4f}: "
              f"{'met' if np.median(t) <= bound else 'NOT met'}", file=out)


if __name__ == "__main__":
    main()
