"""Device times of the varyings resolve (frr_resolve_varyings: k_vary_slots + k_vary_resolve) beside k_raster of the same
frame.  The resolve is bracketed with frr_event_record / frr_event_elapsed_ms (its kernels are not in the profiler's table);
frames are serial and everything runs on the ctx's one stream (frames_in_flight 1, overlap 0, a synchronisation point per
frame), so the two events enclose the two launches and nothing else.  Two cases at 1920x1080: the 69k-triangle sphere
(VS_PHONG, K = 8) under its Phong draw, and a 64,800-triangle grid that covers every pixel (VS_CLIP_COLOR, K = 3).
Beside the times: the bytes a full buffer takes (W * H * K * 4), the bytes the resolve stored (owned pixels only) and the
store rate they give.  Writes what profiles/vary_times.txt holds.

  python tools/vary_times.py [out.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # first, see tests/conftest.py
import numpy as np

import f_renderer_amd as fr
from f_renderer_amd import scenes

WARM, N, REPS = 5, 20, 3


def grid_mesh(gx=240, gy=135):
    """VS_CLIP_COLOR inputs of a gx x gy grid of quads over the whole clip square (two triangles each), z and colour varying"""
    xs, ys = np.linspace(-1.0, 1.0, gx + 1), np.linspace(-1.0, 1.0, gy + 1)
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    Wc = 1.0 + 0.5 * (X * X + Y * Y)
    V = np.stack([X * Wc, Y * Wc, 0.5 * Wc, Wc, 0.5 + 0.5 * X, 0.5 + 0.5 * Y, 0.25 + 0.5 * X * Y], axis=2)
    a, b, c, d = V[:-1, :-1], V[1:, :-1], V[1:, 1:], V[:-1, 1:]
    return np.stack([np.stack([a, b, c], axis=2), np.stack([a, c, d], axis=2)], axis=2).reshape(-1, 3, 7).astype(np.float32)


def measure(r, frame, resolve):
    rows = []
    for rep in range(-1, REPS):
        r.profile_reset()
        ms = []
        for _ in range(WARM if rep < 0 else N):
            frame()
            r.event_record(0)
            resolve()
            r.event_record(1)
            r.sync()
            ms.append(r.event_elapsed_ms(0, 1))
        if rep >= 0:
            t, c = r.profile_get("k_raster")
            rows.append((float(np.mean(ms)) * 1e3, float(np.min(ms)) * 1e3, t / max(c, 1) * 1e3))
    return rows


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    cfg = scenes.build_config("cfg3")
    W, H = cfg["W"], cfg["H"]
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
    print(f"varyings resolve (k_vary_slots + k_vary_resolve, event-bracketed), {W}x{H}, frames serial on one stream (frames_in_flight 1, "
          f"overlap 0, frr_sync per frame), {WARM} warm-up frames, {REPS} x {N} frames; us per frame", file=out)
    cases = (("sphere 69k triangles, VS_PHONG / PS_PHONG, K = 8", cfg["mesh"], fr.VS_PHONG, fr.PS_PHONG, 8),
             ("grid 64,800 triangles over every pixel, VS_CLIP_COLOR / PS_COLOR, K = 3", grid_mesh(), fr.VS_CLIP_COLOR, fr.PS_COLOR, 3))
    for name, mesh, vs, ps, K in cases:
        r = fr.Renderer(W, H)
        r.set_option("frames_in_flight", 1)
        r.set_option("overlap", 0)
        if vs == fr.VS_PHONG:
            r.set_texture(0, cfg["tex"])
            r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye, texture_slot=0)
        m = r.upload_mesh(mesh, vs)
        buf = torch.zeros((W * H, K), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.profile_enable(True, kernels=("k_raster",))

        def frame():
            r.clear()
            r.draw(m, ps)

        def resolve():
            r.resolve_varyings(buf.data_ptr(), W * H)

        frame()
        owned = int((r.readback()[2] != 0xFFFFFFFF).sum())
        full, stored = W * H * K * 4, owned * K * 4
        print(f"\n{name}: {mesh.shape[0]} triangles, {owned} of {W * H} pixels owned; full buffer W*H*K*4 = {full / 1e6:.1f} MB, stored {stored / 1e6:.1f} MB", file=out)
        for rep, (mean_us, min_us, raster_us) in enumerate(measure(r, frame, resolve)):
            print(f"  run {rep}: resolve {mean_us:8.1f} us (min {min_us:8.1f})   k_raster {raster_us:8.1f} us   "
                  f"stores {stored / (mean_us * 1e-6) / 1e9:7.1f} GB/s   (a full buffer at this time: {full / (mean_us * 1e-6) / 1e9:7.1f} GB/s)", file=out)
        r.close()


if __name__ == "__main__":
    main()
