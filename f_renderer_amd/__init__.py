"""f_renderer_amd -- MI355X (gfx950) rasterization path behind f_renderer's Renderer/FrameBuffer
surface.  Python here is plumbing over the C ABI in include/frr.h (libfrr_hip.so); the compute
path is hand-written HIP in f_renderer_amd/csrc.  No CPU fallback exists."""
from . import scenes  # noqa: F401
from ._native import (FRR_ERR_CAPACITY, FRR_ERR_HIP, FRR_ERR_INVALID, FRR_ERR_NOMEM, FRR_ERR_UNSUPPORTED,  # noqa: F401
                      FRR_OK, FrrError, build, lib)
from ._native import PER_ITEM, PER_TRIANGLE, VISIBLE_LDS_BINS  # noqa: F401
from .renderer import (CULL_NEG, CULL_NONE, CULL_POS, PS_BLINN, PS_COLOR, PS_DEPTH, PS_FLAT, PS_PHONG, VS_CLIP,  # noqa: F401
                       VS_CLIP_COLOR, VS_GOURAUD, VS_PHONG, MATERIAL_DTYPE, Camera, DrawList, FrameBuffer, Instances, Lines, Materials, Mesh, Renderer,
                       host_cull_det, host_entry_items, host_instance_mvp, host_list_item, host_query_boxes, host_visible_counts, set_identity, set_look_at, set_perspective)
