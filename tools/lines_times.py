"""Per-launch device times of the line kernels (k_lines_mark, k_lines_paint) beside k_raster of the same frame, with
frr_profile_get: serial frames (one target set, a synchronisation point per frame), warm-up, then REPS x N launches.
Two cases: the wireframe of the headline scene (1M random triangles, 1920x1080) over its depth-only draw, and 10,000
random segments at 1080p over the same draw.  Writes what profiles/lines_times.txt holds.

  python tools/lines_times.py [out.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
try:
    import torch  # noqa: F401  (first, see tests/conftest.py)
except Exception:
    pass
import numpy as np

import f_renderer_amd as fr
from f_renderer_amd import scenes

W, H, NTRIS, NSEG = 1920, 1080, 1_000_000, 10_000
WARM, N, REPS = 5, 20, 3
KERN = ("k_raster", "k_lines_mark", "k_lines_paint")


def measure(r, frame):
    rows = []
    for _ in range(WARM):
        frame()
        r.sync()
    for _ in range(REPS):
        r.profile_reset()
        for _ in range(N):
            frame()
            r.sync()
        rows.append([r.profile_get(k) for k in KERN])
    return rows


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    r = fr.Renderer(W, H)
    r.set_option("frames_in_flight", 1)
    m = r.upload_mesh(scenes.random_clip_triangles(NTRIS, W, H), fr.VS_CLIP)
    g = np.random.default_rng(1)
    xyxy = np.stack([g.integers(0, W, NSEG), g.integers(0, H, NSEG), g.integers(0, W, NSEG), g.integers(0, H, NSEG)], axis=1).astype(np.uint32)
    L = r.upload_lines(xyxy, g.integers(0, 256, (NSEG, 4)).astype(np.uint8))
    px_list = int(sum(1 if dx == dy == 0 else dy if dx == 0 else dx if dy == 0 else dx + dy + 1
                      for dx, dy in zip(np.abs(xyxy[:, 2].astype(np.int64) - xyxy[:, 0]), np.abs(xyxy[:, 3].astype(np.int64) - xyxy[:, 1]))))

    def wire():
        r.clear()
        r.draw(m, fr.PS_DEPTH)
        r.draw_wireframe((255, 255, 255, 255))

    def lines():
        r.clear()
        r.draw(m, fr.PS_DEPTH)
        r.draw_lines(L)

    r.profile_enable(True, kernels=KERN)
    wire()
    setup = r.setup_triangles()
    spi = setup["spi"].astype(np.int64)
    a, b = spi, np.roll(spi, -1, axis=1)
    ok = ((a >= 0) & (b >= 0) & (a < (W, H)) & (b < (W, H))).all(axis=2)
    dx, dy = np.abs(a[..., 0] - b[..., 0])[ok], np.abs(a[..., 1] - b[..., 1])[ok]
    px_wire = int(np.where((dx == 0) & (dy == 0), 1, np.where(dx == 0, dy, np.where(dy == 0, dx, dx + dy + 1))).sum())
    print(f"line kernels, {W}x{H}, frames serial (frames_in_flight 1, frr_sync per frame), {WARM} warm-up frames, {REPS} x {N} launches; us per launch (mean of {N})", file=out)
    for name, frame, nseg, npx in (("wireframe of random_1M_tris_1920x1080", wire, int(ok.sum()), px_wire), (f"{NSEG} random segments", lines, NSEG, px_list)):
        print(f"\n{name}: {nseg} segments drawn ({setup.shape[0] * 3 if frame is wire else nseg} listed), {npx} pixel writes", file=out)
        for rep, row in enumerate(measure(r, frame)):
            print("  run %d: " % rep + "   ".join(f"{k} {t / max(c, 1) * 1e3:8.1f} us x{c}" for k, (t, c) in zip(KERN, row)), file=out)
    r.close()


if __name__ == "__main__":
    main()
