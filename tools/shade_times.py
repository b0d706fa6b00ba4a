"""Device times of shading a varyings buffer (frr_shade_varyings: k_shade_vary) beside the forward frame of the same scene.
Three things per config, each bracketed with frr_event_record / frr_event_elapsed_ms:
  (a) forward   clear + draw(PS_BLINN / PS_PHONG): the frame as the library has always drawn it
  (b) deferred  clear + draw(PS_DEPTH) + resolve_varyings + shade_varyings: the same image, every pixel shaded once
  (c) relight   shade_varyings alone over the buffer of (b): the cost of a new light, eye, texture slot or user uniform
Frames are serial and everything runs on the ctx's one stream (frames_in_flight 1, overlap 0, a synchronisation point per
frame), so two events enclose the launches between them and nothing else.  The three are measured in one process,
alternating, and reported as the median over the runs (each run: the mean of N frames).  Beside the times: the traffic bound
W*H*(4 + 4*K*f + 4*f) bytes (ids in, f = drawn share: varyings in, colour out) and the rate it gives for (c).
Configs: the 4K textured Blinn frame (cfg5) and the 69k-triangle Phong sphere at 1080p (cfg3).  Writes what
profiles/shade_times.txt holds.

  python tools/shade_times.py [out.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # first, see tests/conftest.py
import numpy as np

import f_renderer_amd as fr
from f_renderer_amd import scenes

WARM, N, RUNS = 5, 20, 5


def timed(r, body):
    """mean us per frame of N frames of `body`"""
    ms = []
    for _ in range(N):
        r.event_record(0)
        body()
        r.event_record(1)
        r.sync()
        ms.append(r.event_elapsed_ms(0, 1))
    return float(np.mean(ms)) * 1e3


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    print(f"shading a varyings buffer (k_shade_vary, event-bracketed) beside the forward frame; frames serial on one stream "
          f"(frames_in_flight 1, overlap 0, frr_sync per frame), {WARM} warm-up frames each, {RUNS} alternating runs of {N} frames; "
          f"us per frame, median over the runs (min .. max)", file=out)
    for name in ("cfg5", "cfg3"):
        cfg = scenes.build_config(name)
        W, H, mesh = cfg["W"], cfg["H"], cfg["mesh"]
        ps = getattr(fr, "PS_" + cfg["ps"])
        K = 8
        eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
        r = fr.Renderer(W, H)
        r.set_option("frames_in_flight", 1)
        r.set_option("overlap", 0)
        r.set_texture(0, cfg["tex"])
        r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye, texture_slot=0)
        m = r.upload_mesh(mesh, fr.VS_PHONG)
        buf = torch.zeros((W * H, K), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def forward():
            r.clear()
            r.draw(m, ps)

        def deferred():
            r.clear()
            r.draw(m, fr.PS_DEPTH)
            r.resolve_varyings(buf.data_ptr(), W * H)
            r.shade_varyings(ps, buf.data_ptr(), W * H, K)

        def relight():
            r.shade_varyings(ps, buf.data_ptr(), W * H, K)

        forward()
        want, _, ids = r.readback()
        deferred()
        got = r.readback()[0]
        same = bool((got == want).all())
        f = float((ids != 0xFFFFFFFF).mean())
        bound = W * H * (4 + 4 * K * f + 4 * f)
        bodies = {"forward": forward, "deferred": deferred, "relight": relight}
        for body in bodies.values():
            for _ in range(WARM):
                body()
            r.sync()
        runs = {k: [] for k in bodies}
        for _ in range(RUNS):
            for k, body in bodies.items():
                runs[k].append(timed(r, body))
        st = r.stats()
        print(f"\n{name}: {W}x{H}, {mesh.shape[0]} triangles, PS_{cfg['ps']}, K = {K}; drawn share f = {f:.3f}; covered fragments per frame {st['frag_covered']}; "
              f"deferred image == forward image: {same}", file=out)
        print(f"  traffic bound of the shade W*H*(4 + 4*K*f + 4*f) = {bound / 1e6:.1f} MB", file=out)
        for k, label in (("forward", "(a) forward  clear + draw(shaded)              "), ("deferred", "(b) deferred clear + draw(depth) + resolve + shade"),
                         ("relight", "(c) relight  shade alone                          ")):
            v = runs[k]
            line = f"  {label} {np.median(v):9.1f} us  ({min(v):9.1f} .. {max(v):9.1f})"
            if k == "relight":
                line += f"   = {bound / (np.median(v) * 1e-6) / 1e9:7.1f} GB/s of the traffic bound"
            print(line, file=out)
        r.close()


if __name__ == "__main__":
    main()
