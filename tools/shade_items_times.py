"""Device times of shading all the items of a list pass under their own materials (frr_shade_items: k_shade_items) beside the
only way there was before it.  Per scene, at 1920 x 1080, VS_PHONG / PS_PHONG, over one depth-only list pass and one
resolve_varyings made before the clock starts; each bracketed with frr_event_record / frr_event_elapsed_ms:
  (a) items    one shade_items over the pass's material table
  (b) loop     for every item { set_uniforms(texture_slot, strengths, flat colour) ; shade_varyings(ids of the item) }: one pass
               over every pixel of the window per item
  (c) floor    one unranged shade_varyings under a single material: the same pixels, no lookup
Frames are serial and everything runs on the ctx's one stream (frames_in_flight 1, overlap 0, a synchronisation point per
frame), so two events enclose the launches between them and nothing else -- for (b) that includes the gaps in which the device
waits for the host to issue the next call.  The three are measured in one process, alternating, and reported as the median
over the runs (each run: the mean of N frames).  Beside the times: the histogram of DISTINCT items per 64-entry span of the
frame's ids (frr_host_entry_items: a span shades once per distinct item, so it is what (a) / (c) should follow).
Scenes: (i) and (ii) of tools/drawlist_times.py, and its (iii): three large, different meshes, the shape of phong.rs:319-359.
Writes what profiles/shade_items_times.txt holds.

  python tools/shade_items_times.py [out.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first, see tests/conftest.py)
import numpy as np  # noqa: E402

import f_renderer_amd as fr  # noqa: E402
from f_renderer_amd import scenes  # noqa: E402
from tools.drawlist_times import configs  # noqa: E402
from tools.instanced_times import H, W, grid_models  # noqa: E402
from tools.shade_times import N, RUNS, WARM, timed  # noqa: E402

NONE = 0xFFFFFFFF


def materials(n):
    m = np.zeros(n, fr.MATERIAL_DTYPE)
    k = np.arange(n)
    m["texture_slot"] = k % 3
    m["ambient_strength"] = (0.05 + 0.1 * (k % 5)).astype(np.float32)
    m["specular_strength"] = (0.2 + 0.15 * (k % 4)).astype(np.float32)
    m["flat_color"] = 1.0
    return m


def span_histogram(items):
    """{distinct items in a 64-entry span: number of spans} of an [H, W] item array (W a multiple of 64)"""
    s = np.sort(items.reshape(-1, 64).astype(np.int64), axis=1)
    distinct = (np.diff(s, axis=1) != 0).sum(axis=1) + 1 - (s[:, -1] == NONE)   # (NONE, the largest value, is no item)
    vals, counts = np.unique(distinct, return_counts=True)
    return {int(v): int(c) for v, c in zip(vals, counts)}


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    print(f"shading the items of a list pass under their own materials (k_shade_items, event-bracketed) beside one ranged shade_varyings per "
          f"item and beside one unranged shade_varyings; {W} x {H}, PS_PHONG, K = 8; frames serial on one stream (frames_in_flight 1, overlap 0, "
          f"frr_sync per frame), {WARM} warm-up frames each, {RUNS} alternating runs of {N} frames; us per frame, median over the runs (min .. max)", file=out)
    assert W % 64 == 0
    base = scenes.checker_texture(256, 16)
    texs = [base, base.copy(), base.copy()]
    texs[1][..., 0], texs[2][..., 1] = 255 - base[..., 0], 255 - base[..., 1]
    for name, meshes, nitems, _ in configs():
        models = grid_models(nitems)
        which = (np.arange(nitems) * 7 + np.arange(nitems) // len(meshes)) % len(meshes)
        eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
        r = fr.Renderer(W, H)
        r.set_option("frames_in_flight", 1)
        r.set_option("overlap", 0)
        for slot, t in enumerate(texs):
            r.set_texture(slot, np.ascontiguousarray(t))
        r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye, texture_slot=0)
        ms = [r.upload_mesh(m, fr.VS_PHONG) for m in meshes]
        lst = r.upload_draw_list([ms[w] for w in which], models)
        mats = materials(nitems)
        tab = r.upload_materials(mats)
        buf = torch.zeros((W * H, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.clear()
        r.draw_list(lst, fr.PS_DEPTH)
        r.resolve_varyings(buf.data_ptr(), W * H)
        first, count = r.item_ranges()
        ids = r.readback()[2]

        def call_uniforms():
            r.set_uniforms(texture_slot=0, ambient_strength=np.float32(0.1), specular_strength=0.5)

        def items():
            r.shade_items(fr.PS_PHONG, buf.data_ptr(), tab, W * H, 8)

        def loop():
            for k in range(nitems):
                r.set_uniforms(texture_slot=int(mats["texture_slot"][k]), ambient_strength=mats["ambient_strength"][k], specular_strength=mats["specular_strength"][k])
                r.shade_varyings(fr.PS_PHONG, buf.data_ptr(), W * H, 8, ids=(int(first[k]), int(count[k])))
            call_uniforms()

        def floor():
            r.shade_varyings(fr.PS_PHONG, buf.data_ptr(), W * H, 8)

        items()
        ca = r.readback()[0]
        loop()
        cl = r.readback()[0]
        same = bool((ca == cl).all())
        bounds = np.concatenate([first.astype(np.int64), [int(first[-1]) + int(count[-1])]])
        item, rounds = fr.host_entry_items(ids, (0, W), (0, H), bounds)
        hist = span_histogram(item.reshape(H, W))
        spans = sum(hist.values())
        assert rounds == sum(k * v for k, v in hist.items())
        bodies = {"items": items, "loop": loop, "floor": floor}
        for body in bodies.values():
            for _ in range(WARM):
                body()
            r.sync()
        runs = {k: [] for k in bodies}
        for _ in range(RUNS):
            for k, body in bodies.items():
                runs[k].append(timed(r, body))
        f = float((ids != NONE).mean())
        print(f"\n{name}: {nitems} items, tris_setup {r.stats()['tris_setup']}, drawn share f = {f:.3f}; shade_items frame == loop frame (colour): {same}", file=out)
        for k, label in (("items", "(a) items  one shade_items                  "), ("loop", f"(b) loop   {nitems:5d} ranged shade_varyings      "),
                         ("floor", "(c) floor  one unranged shade_varyings      ")):
            v = runs[k]
            print(f"  {label} {np.median(v):11.1f} us  ({min(v):11.1f} .. {max(v):11.1f})", file=out)
        a, b, c = (float(np.median(runs[k])) for k in ("items", "loop", "floor"))
        print(f"  (b) / (a) = {b / a:.1f}   (a) / (c) = {a / c:.2f}   (a) {'below' if a < b else 'NOT below'} (b)", file=out)
        nonempty = spans - hist.get(0, 0)
        print(f"  distinct items per 64-entry span: {spans} spans, {hist.get(0, 0)} hold no id of the pass; of the other {nonempty}: "
              + ", ".join(f"{k}: {v}" for k, v in sorted(hist.items()) if k) + f"; rounds = {rounds}, {rounds / max(nonempty, 1):.2f} per span that shades", file=out)
        r.close()


if __name__ == "__main__":
    main()
