"""Times of face culling (frr_set_cull), one frame at a time (run with FRR_FRAMES_IN_FLIGHT=1 FRR_OVERLAP=0): per-kernel device
times from frr_profile_get (k_geom, k_bin_seg, k_raster) and the frame period from device events around 20 frames, fragment counting
off as in bench.py's timed frames (the statistics beside them are of a counted frame).

  python tools/cull_times.py off                 one JSON line: headline and cfg3 at full size with culling off -- run it with
                                                 FRR_LIB pointing at a build of the parent commit and at this build in turn
                                                 (the parent has no frr_set_cull: its two symbols are then not looked up)
  python tools/cull_times.py on                  cfg2 (torus, CULL_NEG) and cfg3 (sphere, CULL_POS) at full size, culled against
                                                 unculled, kernel by kernel, with tris_setup / bin_entries / frag_covered
  python tools/cull_times.py report PARENT.jsonl THIS.jsonl
                                                 medians and spreads of the `off` lines of the two builds, and the condition:
                                                 this build's median k_geom time and frame period are no higher than the
                                                 parent's median plus the parent's own min-to-max spread
profiles/cull_times.txt holds the output of `on` and of `report`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_geom", "k_bin_seg", "k_raster")
FRAMES = 20


def renderer(fr, scenes, cfg):
    W, H = cfg["W"], cfg["H"]
    r = fr.Renderer(W, H)
    if cfg["cam"]:
        eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
        r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye)
    if cfg["tex"] is not None:
        r.set_texture(0, cfg["tex"])
        r.set_uniforms(texture_slot=0)
    r.set_uniforms(flat_color=cfg["flat_color"])
    return r


def measure(r, m, ps):
    """{period_us, k_geom, k_bin_seg, k_raster (us per launch), stats} of clear + draw(m)"""
    def frame():
        r.clear()
        r.draw(m, ps)
    for _ in range(3):
        frame()
    r.sync()
    st = r.stats()
    r.set_count_fragments(False)   # (as bench.py times its frames; the statistics above are of a counted frame)
    periods = []
    for _ in range(3):
        r.event_record(0)
        for _ in range(FRAMES):
            frame()
        r.event_record(1)
        periods.append(r.event_elapsed_ms(0, 1) / FRAMES * 1e3)
    out = {"period_us": min(periods), "stats": {k: st[k] for k in ("tris_in", "tris_setup", "bin_entries", "frag_covered")}}
    r.profile_enable(True, kernels=list(KERNELS))
    r.profile_reset()
    for _ in range(FRAMES):
        frame()
    r.sync()
    for k in KERNELS:
        ms, n = r.profile_get(k)
        out[k] = ms / n * 1e3 if n else 0.0
    r.profile_enable(False)
    r.set_count_fragments(True)
    return out


def off():
    from f_renderer_amd import _native
    import ctypes
    if os.environ.get("FRR_LIB") and not hasattr(ctypes.CDLL(os.environ["FRR_LIB"]), "frr_set_cull"):
        for s in ("frr_set_cull", "frr_host_cull_det"):
            _native.SIGNATURES.pop(s)
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    res = {"lib": os.path.basename(os.environ.get("FRR_LIB", "in-tree"))}
    for name in ("headline", "cfg3"):
        cfg = scenes.build_config(name)
        r = renderer(fr, scenes, cfg)
        res[name] = measure(r, r.upload_mesh(cfg["mesh"], getattr(fr, "VS_" + cfg["vs"])), getattr(fr, "PS_" + cfg["ps"]))
        r.close()
    print(json.dumps(res), flush=True)


def on():
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    print(f"culled against unculled at full size, one frame at a time; device time per launch from frr_profile_get over {FRAMES} frames, frame "
          f"period = device events around {FRAMES} frames (best of 3), fragment counting off")
    for name, mode, label in (("cfg2", fr.CULL_NEG, "CULL_NEG"), ("cfg3", fr.CULL_POS, "CULL_POS")):
        cfg = scenes.build_config(name)
        r = renderer(fr, scenes, cfg)
        m, ps = r.upload_mesh(cfg["mesh"], getattr(fr, "VS_" + cfg["vs"])), getattr(fr, "PS_" + cfg["ps"])
        rows = {}
        for tag, md in (("unculled", fr.CULL_NONE), (label, mode), ("unculled again", fr.CULL_NONE)):
            r.set_cull(md)
            rows[tag] = measure(r, m, ps)
        print(f"\n{name} ({cfg['W']} x {cfg['H']}, {cfg['mesh'].shape[0]} triangles, VS_{cfg['vs']} / PS_{cfg['ps']})")
        for tag, v in rows.items():
            s = v["stats"]
            print(f"  {tag:15s} k_geom {v['k_geom']:7.1f} us  k_bin_seg {v['k_bin_seg']:7.1f} us  k_raster {v['k_raster']:7.1f} us  period {v['period_us']:7.1f} us"
                  f"  | tris_setup {s['tris_setup']:7d}  bin_entries {s['bin_entries']:8d}  frag_covered {s['frag_covered']:9d}")
        a, b = rows["unculled"], rows[label]
        print("  culled / unculled: " + "  ".join(f"{k} {b[k] / a[k]:.2f}" for k in KERNELS + ("period_us",)) +
              "  | " + "  ".join(f"{k} {b['stats'][k] / max(a['stats'][k], 1):.2f}" for k in ("tris_setup", "bin_entries", "frag_covered")))
        r.close()


def report(parent, this):
    import numpy as np
    runs = {tag: [json.loads(x) for x in open(p) if x.strip().startswith("{")] for tag, p in (("parent", parent), ("this", this))}
    print(f"culling off, this build against the parent commit built the same way: {len(runs['parent'])} and {len(runs['this'])} alternating runs, "
          f"one frame at a time, fragment counting off; median (min .. max)")
    ok = True
    for name in ("headline", "cfg3"):
        print(f"\n{name}")
        for key in ("k_geom", "k_bin_seg", "k_raster", "period_us"):
            v = {tag: [x[name][key] for x in rs] for tag, rs in runs.items()}
            line = f"  {key:10s}" + "".join(f"  {tag} {np.median(x):8.2f} us ({min(x):8.2f} .. {max(x):8.2f})" for tag, x in v.items())
            if key in ("k_geom", "period_us"):
                bound = np.median(v["parent"]) + (max(v["parent"]) - min(v["parent"]))
                met = bool(np.median(v["this"]) <= bound)
                ok = ok and met
                line += f"  bound {bound:8.2f} us: {'met' if met else 'NOT met'}"
            print(line)
    print(f"\ncondition (k_geom and frame period of headline and cfg3): {'met' if ok else 'NOT met'}")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "report":
        report(sys.argv[2], sys.argv[3])
    else:
        import torch  # noqa: F401  (first, see tests/conftest.py)
        {"off": off, "on": on}[what]()
