"""Dev tool: two 64 x 48 frames that use every command kind once (geometry, raster, line list, wireframe, resolve, shade,
visible count; then, behind a list pass of two items and its raster pass, the per-item shade over a table of two materials
and the occlusion query per item; last, the box query over a list of two lit items, whose bounds are computed before the frames),
for a kernel trace that shows what the host layer dispatches, in order:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python3 tools/trace_commands.py
  python3 tools/trace_commands.py --names DIR/.../kt_kernel_trace.csv > names.txt     (kernel names by dispatch id)"""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def names(path):
    with open(path) as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        print(r["Kernel_Name"])


def frames():
    import torch  # noqa: F401  (first: it bundles its own HIP runtime)
    import numpy as np
    import f_renderer_amd as fr
    from f_renderer_amd import scenes

    W, H = 64, 48
    r = fr.Renderer(W, H)
    mesh = r.upload_mesh(scenes.single_triangle_rgb(), fr.VS_CLIP_COLOR)
    lines = r.upload_lines(np.array([[1, 1, 40, 30]], np.uint32), np.array([[255, 255, 0, 255]], np.uint8))
    items = r.upload_draw_list([mesh, mesh], np.stack([np.eye(4, dtype=np.float32)] * 2))
    mats = r.upload_materials([{"flat_color": (1, 0, 0, 1)}, {"flat_color": (0, 1, 0, 1)}])
    lit = r.upload_mesh(scenes.torus(4, 4), fr.VS_PHONG)
    boxed = r.upload_draw_list([lit, lit], np.stack([np.eye(4, dtype=np.float32)] * 2))
    r.list_bounds(boxed)
    vary = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    counts = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):
        r.clear()
        r.geometry_processing(mesh)
        r.rasterization((0, W), (0, H), fr.PS_DEPTH)
        r.draw_lines(lines)
        r.draw_wireframe((255, 0, 0, 255))
        r.resolve_varyings(vary.data_ptr(), W * H)
        r.shade_varyings(fr.PS_COLOR, vary.data_ptr())
        r.visible_pixels("item", out_ptr=counts.data_ptr(), entries=4)
        r.geometry_list(items)
        r.rasterization((0, W), (0, H), fr.PS_DEPTH)
        r.shade_items(fr.PS_COLOR, vary.data_ptr(), mats)
        r.query_pixels("item", out_ptr=counts.data_ptr(), entries=4)
        r.query_boxes(boxed, out_ptr=counts.data_ptr(), entries=4)
        r.sync()
    c, _, t = r.readback()
    print("drawn pixels", int((t != 0xFFFFFFFF).sum()), "colour sum", int(c.sum()))
    r.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--names":
        names(sys.argv[2])
    else:
        frames()
