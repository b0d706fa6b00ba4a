/*
 * frr.h -- C ABI of libfrr_hip.so: the MI355X (gfx950) rasterization path behind
 * vmskisme/f_renderer's Renderer / FrameBuffer surface.
 *
 * The reference API is per-triangle and closure-based (Rust generics):
 *   Renderer::geometry_processing   /root/reference/f_renderer/src/renderer.rs:96-112
 *   Renderer::rasterization         /root/reference/f_renderer/src/renderer.rs:269-284
 *   FrameBuffer::{new,fill,clear,get_data,get_size,set_pixel,get_pixel,sample_2d,draw_line}
 *                                   /root/reference/f_renderer/src/renderer.rs:418-588
 * driven by the two-pass draw loop   /root/reference/examples/src/bin/phong.rs:314-387.
 * Closures and generic varyings cannot cross an FFI to a GPU, so this ABI is batched at the
 * granularity of that draw loop and shaders are table-selected; varyings are a flat float[K]
 * (the trait bounds Add+Sub+Mul<f32>+Copy+Default, renderer.rs:97-102, say "K-dim real vector").
 * Plain pointers and sizes only; no torch / C++ types.  All functions return FRR_OK (0) or a
 * negative frr_status; nothing unwinds across this boundary.  A frr_ctx is driven by one host
 * thread (the reference is single-threaded, vulkan_base.rs:698-723).
 *
 * There is NO CPU fallback behind these symbols: every entry point that computes needs a gfx950
 * device and fails with FRR_ERR_HIP otherwise.
 */
#ifndef FRR_H
#define FRR_H
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define FRR_ABI_VERSION 4
#define FRR_MAX_VARYINGS 16
#define FRR_MAX_TEXTURES 4
#define FRR_MAX_USER_UNIFORMS 64 /* f32 a user shader receives (frr_set_user_uniforms) */
#define FRR_SHADER_USER_BASE 64  /* ids of user shaders (frr_shader_register) start here */
#define FRR_MAX_OUT_TRIS 19 /* 3 + 18 clip vertices -> 19 fan triangles (renderer.rs:150-171,245-264) */

typedef struct frr_ctx frr_ctx;

typedef enum frr_status {
    FRR_OK = 0,
    FRR_ERR_INVALID = -1,     /* bad argument (the reference would panic: clamp min>max, OOB index) */
    FRR_ERR_HIP = -2,         /* HIP runtime error / no gfx950 device; see frr_last_error */
    FRR_ERR_NOMEM = -3,
    FRR_ERR_UNSUPPORTED = -4,
    FRR_ERR_CAPACITY = -5     /* not something a caller has to handle: a device work list (fan slots, (triangle, tile)
                                 records) that turns out too small is grown and the commands since the failing one are
                                 replayed INSIDE the library at the next synchronisation point (frr_sync, frr_readback,
                                 frr_get_stats ...) -- Renderer::rasterization cannot fail (renderer.rs:269-384), neither
                                 can frr_draw.  This code is returned only if eight replays in a row were not enough. */
} frr_status;

/* Vertex-shader table.  Replaces the `vertex_shader: &F` closure argument (renderer.rs:105,110). */
typedef enum frr_vs {
    FRR_VS_CLIP = 0,       /* VSInput = clip xyzw (4 f32);               K = 0 */
    FRR_VS_CLIP_COLOR = 1, /* VSInput = clip xyzw + rgb (7 f32);         K = 3 */
    FRR_VS_PHONG = 2,      /* VSInput = pos3,uv2,normal3 (phong.rs:49-54); body phong.rs:114-126; K = 8 */
    FRR_VS_GOURAUD = 3     /* same input; per-vertex Lambert colour;     K = 3 */
} frr_vs;

/* Pixel-shader table.  Replaces the `pixel_shader: &F` closure argument (renderer.rs:273,283). */
typedef enum frr_ps {
    FRR_PS_DEPTH = 0, /* depth (+triangle id) only, colour untouched */
    FRR_PS_FLAT = 1,  /* uniforms.flat_color */
    FRR_PS_COLOR = 2, /* (ctx[0],ctx[1],ctx[2],1) */
    FRR_PS_PHONG = 3, /* phong.rs:133-154 (reflect-vector Phong x bilinear texture) */
    FRR_PS_BLINN = 4  /* half-vector variant of the same (not in the reference) */
} frr_ps;

/* Face-cull mode of the geometry passes (frr_set_cull), named by the sign of the determinant it drops. */
typedef enum frr_cull {
    FRR_CULL_NONE = 0, /* every input is processed (the reference's behaviour, and the default) */
    FRR_CULL_NEG = 1,  /* drop inputs with d < 0 */
    FRR_CULL_POS = 2   /* drop inputs with d > 0 */
} frr_cull;

/* ---- user shaders -------------------------------------------------------------------------------------------
 * The reference's shaders are closures: `vertex_shader: &F` with F: Fn(&VSUniform, &VSInput, &mut ShaderContext) -> Vec4
 * (renderer.rs:105,110,116) and `pixel_shader: &F` with F: Fn(&PSUniform, &ShaderContext) -> Vec4 (:273,283,380), over any
 * varying type that is a real vector space (Add + Sub + Mul<f32> + Copy + Default, :97-102).  A closure cannot cross this
 * boundary as a function pointer -- it has to run on the GPU inside the geometry and tile kernels -- so it crosses as
 * TEXT: HIP device source that the library compiles at run time (hiprtc, gfx950, -ffp-contract=off like the library
 * itself) into its own kernels.  The source defines, at global scope,
 *
 *   __device__ void frr_user_vs(const frr::DevUniforms &u, const float *in, float pos[4], float *ctx);
 *       in: vs_input_floats f32 of one vertex;  ctx: num_varyings f32, zero on entry (T::default());  pos: clip xyzw
 *   __device__ void frr_user_ps(const frr::DevUniforms &u, const float *ctx, float out[4], const float *u8lut);
 *       ctx: the interpolated varyings (renderer.rs:374-378);  out: the Vec4 that vec4_to_u8_array quantises (:7-14)
 *
 * and may use what the built-in shaders are written with (f_renderer_amd/csrc/frr_device.h, frr_exact.h, namespace frr):
 * u.mvp / u.model (column-major), u.view_pos, u.light_pos, u.light_color, u.ambient_strength, u.specular_strength,
 * u.flat_color, u.user[FRR_MAX_USER_UNIFORMS] (frr_set_user_uniforms: what the closure would have captured),
 * frr::mat4_mul_vec4, frr::dot3, frr::normalize3 (glam's operation order), frr::f32_max, frr::recip_exact, and
 * frr::sample_2d(u, uu, vv, rgba_out, u8lut) (FrameBuffer::sample_2d of the texture in uniforms.texture_slot, :516-538) and
 * frr::sample_2d_slot(u, slot, uu, vv, rgba_out, u8lut) (the same of ANY uploaded slot 0..FRR_MAX_TEXTURES-1: the
 * reference's PSUniform holds three textures and its closure may sample each, phong.rs:41-47,147-151; an empty slot
 * samples as zero).  fp32 expressions keep their written association (no FMA contraction), as in the reference's Rust.
 *
 * frr_shader_register returns one id >= FRR_SHADER_USER_BASE that stands for the pair: pass it as vs_id to
 * frr_mesh_upload / frr_mesh_bind_device and as ps_id to frr_raster / frr_draw.  The two halves also combine with the
 * tables: a mesh uploaded with a user id may be drawn with a built-in ps_id, and a mesh with a built-in (or another
 * user) vs_id with a user ps_id -- provided the pixel shader's varyings are the vertex shader's (frr_vs_num_varyings;
 * FRR_ERR_INVALID otherwise).  ctx may be NULL (compile only: the registry is per process; a ctx loads the code object
 * on first use).  A source that does not compile: FRR_ERR_UNSUPPORTED, with the compiler's log in frr_last_error(ctx). */
int frr_shader_register(frr_ctx *ctx, const char *hip_source, int vs_input_floats, int num_varyings, int *shader_id);
/* u.user[0..n) for the draws issued from now on (n <= FRR_MAX_USER_UNIFORMS; travels with each draw like frr_uniforms) */
int frr_set_user_uniforms(frr_ctx *ctx, const float *values, int n);

/* VSUniform (phong.rs:26-31) + PSUniform (phong.rs:41-47) + light consts (phong.rs:128-132).
 * Matrices column-major like glam::Mat4::from_cols_array (matrix_util.rs:5-7). */
typedef struct frr_uniforms {
    float model[16], view[16], proj[16];
    float view_pos[3];
    float light_pos[3];
    float light_color[3];
    float ambient_strength;
    float specular_strength;
    float flat_color[4];
    int32_t texture_slot; /* PSUniform.place (phong.rs:34-38,147-151) */
} frr_uniforms;

/* One post-setup vertex as the parity tests read it back: the caller-visible content of
 * Vertex<T> (renderer.rs:387-394) minus the NDC `pos`, in EMISSION order (before the
 * orientation swap of renderer.rs:309-312). */
typedef struct frr_setup_vertex {
    float spf[2];
    int32_t spi[2];
    float rhw;
    float ctx[FRR_MAX_VARYINGS];
} frr_setup_vertex;

typedef struct frr_stats {
    uint64_t tris_in;      /* input triangles submitted since the last frr_clear */
    uint64_t tris_setup;   /* triangles after clip + fan */
    uint64_t bin_entries;  /* (triangle, tile) pairs */
    uint64_t frag_covered; /* pass the edge tests renderer.rs:333-341 (exact only while counting is enabled) */
    uint64_t frag_nan;     /* fragments whose rhw interpolated to NaN; they always pass the depth test and so does the next
                              fragment on their pixel (renderer.rs:363-366): reproduced exactly, by a second pass over the
                              tiles that saw one (the NaN bit pattern itself is the device's) */
    uint32_t draws;        /* On a partitioned ctx (frr_set_partition, world > 1) tris_in, tris_setup and draws are those of the
                              unpartitioned frame on every rank (geometry is replicated), while frag_covered and frag_nan are
                              counted by the tile kernels of the tiles the rank owns: the ranks' sums are the unpartitioned
                              figures */
    uint32_t replays;      /* how often the library had to grow a work list and replay commands of this frame (see
                              FRR_ERR_CAPACITY): a diagnostic, the results are those of a frame that never failed */
} frr_stats;

/* ---- context ------------------------------------------------------------------------------ */

/* Creates a context on HIP device `device` with a width x height FrameBuffer (renderer.rs:419-425),
 * an f32 depth buffer (phong.rs:208) and a u32 triangle-id buffer.  `stream` is a hipStream_t the
 * caller owns (e.g. torch's current stream), or NULL for a private stream: everything that touches the frame targets
 * (tile kernels, clears, read-backs) runs on it, in call order.  The ctx owns a second, private stream on which the
 * geometry and binning kernels of the next draw run beside the tile kernel of the current one (option "overlap");
 * it is ordered against `stream` with events, so the caller sees one in-order queue -- with one rule: the contents of
 * a device-bound mesh (frr_mesh_bind_device) are read some time between the frr_draw call and the end of the frame's
 * tile kernels, on the library's streams.  A caller that rewrites such a mesh in place therefore (1) orders the rewrite
 * BEHIND the draws issued so far -- frr_frame_fence(ctx, the stream it rewrites on) -- and (2) binds the mesh again
 * (frr_mesh_bind_device: the library's streams then wait for that stream once) before the next draw.  frr_sync in place
 * of (1) and (2) is always sufficient: frr_sync before the rewrite, and again after it when the rewrite is on a stream
 * other than the ctx's or the next draw follows it without a host wait.  (The library does not trust what it learnt
 * about a device-bound mesh's passes across a frr_sync: the next pass of it is verified again -- frr_frame_fence.) */
int frr_create(int device, uint32_t width, uint32_t height, void *stream, frr_ctx **out);
void frr_destroy(frr_ctx *ctx);
const char *frr_last_error(const frr_ctx *ctx);
int frr_abi_version(void);

/* Screen-tile partition for multi-GPU runs: this ctx rasterizes only tile rows ty with
 * ty % world == rank (geometry is replicated).  Default (0,1) = everything. */
int frr_set_partition(frr_ctx *ctx, int rank, int world);
/* Which tile rows a rank owns: 0 (default) = interleaved, ty % world == rank -- balances scenes whose
 * load varies down the screen; 1 = blocked, rank owns a contiguous run of tile_rows / world rows, the first
 * tile_rows % world ranks one more (34 rows over 8 ranks: 5,5,4,4,4,4,4,4; frr_owned_rows tells) -- its part of a
 * row-major image is then ONE contiguous slab, so the final-image gather needs no staging copies (bench.py uses this).
 * tile_rows is counted per command: frr_raster / frr_draw*, frr_resolve_varyings, frr_shade_varyings, frr_shade_items and
 * frr_visible_pixels count the tile rows of their WINDOW (y1 - y0 rows), frr_draw_lines and frr_draw_wireframe those of the
 * ctx (its height).  Interleaved the count does not enter the rule.  Blocked, the two kinds of command own the same rows only
 * in a window with as many tile rows as the ctx (every full-height window): see frr_draw_lines. */
int frr_set_partition_layout(frr_ctx *ctx, int blocked);
/* The pixel rows of a raster window height_range = (y0, y1) (renderer.rs:271: the sub-window argument this whole
 * partition rests on) that this rank owns, as bands [row0, row1) of window-local rows: ONE band in the blocked
 * layout, one per owned 32-pixel tile row in the interleaved layout; a rank that owns nothing has none.  With
 * frr_target_ptrs this is all a non-Python host needs for the final-image exchange: the rank's part of a
 * row-major target of row stride S bytes per row is [row0 * S, row1 * S) of each plane (ncclSend / ncclRecv or
 * peer stores).  frr_owned_band_count returns the number of bands (>= 0) or a negative
 * frr_status. */
int frr_owned_band_count(const frr_ctx *ctx, int32_t y0, int32_t y1);
int frr_owned_rows(const frr_ctx *ctx, int32_t y0, int32_t y1, int32_t band, int32_t *row0, int32_t *row1);
/* The same rule for ANY rank, without a ctx: what the root of the final-image exchange posts its receives with
 * (examples/gather_rccl.cpp).  Returns the number of bands rank `rank` of `world` owns in a window of height_range
 * (y0, y1) (negative: bad argument); if row0/row1 are not NULL and band is in range they receive band `band`. */
int frr_partition_rows(int32_t y0, int32_t y1, int rank, int world, int blocked, int32_t band, int32_t *row0, int32_t *row1);
/* The final-image exchange of one plane as a list of operations -- a pure function of (window, partition, rank), no ctx and
 * no device: what examples/gather_rccl.cpp posts inside one ncclGroupStart / ncclGroupEnd per frame, and what a test can
 * check for every rank of any world size without owning that many GPUs.  The plane is row-major with `row_elems` elements
 * per pixel row; offsets and counts are in elements.  For rank `rank`: on a rank other than `root` one FRR_XFER_SEND per
 * owned band (to root); on root one FRR_XFER_RECV per owned band of every other rank, and one FRR_XFER_COPY per band of its
 * own (render target -> final image, a device copy).  Every element of the window's plane is the destination of exactly
 * one RECV or COPY of root's list, and each SEND of rank p equals (offset, count) the RECV root posts for p, in the same
 * order.  Returns the number of operations (written up to `cap`), or a negative frr_status. */
typedef enum frr_xfer_kind { FRR_XFER_SEND = 0, FRR_XFER_RECV = 1, FRR_XFER_COPY = 2 } frr_xfer_kind;
typedef struct frr_xfer {
    int32_t kind;     /* frr_xfer_kind */
    int32_t peer;     /* SEND: root; RECV: the sending rank; COPY: root itself */
    uint64_t offset;  /* first element, in the rank's render target AND in the final image (same layout), counted from the
                         WINDOW's first row: row 0 of the plane is pixel row y0 of the screen (a window is addressed locally,
                         renderer.rs:323; frr_raster below), so the plan depends on y1 - y0 only */
    uint64_t count;   /* elements */
} frr_xfer;
int frr_exchange_plan(int32_t y0, int32_t y1, uint32_t row_elems, int rank, int world, int blocked, int root, frr_xfer *ops, int cap);
/* frr_stats.frag_covered is exact while counting is enabled (default).  Disabling it lets the tile
 * kernel drop whole triangles by hierarchical early-z before their coverage is known (images are
 * identical either way; only the statistic stops being maintained). */
int frr_set_count_fragments(frr_ctx *ctx, int enable);

/* Use caller-owned DEVICE buffers (e.g. torch tensors) as the frame targets instead of the
 * internally allocated ones; any may be NULL to keep the internal one (with option bound_targets_in_flight: all three
 * or none).  On a partitioned ctx
 * (frr_set_partition, world > 1) only the tile rows the rank owns are defined in caller-owned targets
 * (a clear that was performed inside a draw never touches the other ranks' rows, one that was not -- in front of a
 * sub-window raster or of any other command, or under option clear_eager -- clears the whole target); the ctx's own targets
 * are brought up to date in full whenever they are read back: at frr_readback, and behind frr_target_ptrs and
 * frr_frame_fence, every row and depth / id entry of another rank holds the frame's clear values, never a fragment. */
int frr_bind_targets(frr_ctx *ctx, void *color_rgba8, void *depth_f32, void *tri_id_u32);
/* The device pointers of the current frame's targets, for reads queued on the ctx's stream (which first waits for the
 * frames issued so far).  With two frames in flight the ctx's own targets are two sets: the pointers are those of the
 * CURRENT frame and stay that frame's until the second frr_clear from now, which -- like every frr_clear that reuses a
 * set whose pointers were handed out -- orders the new frame behind what that stream holds by then (the caller's reads). */
int frr_target_ptrs(frr_ctx *ctx, void **color_rgba8, void **depth_f32, void **tri_id_u32);

/* ---- scene ------------------------------------------------------------------------------- */

/* Vec<[VSInput;3]> (phong.rs:187-205): ntris x 3 x floats_per_vertex(vs) f32, host memory. */
int frr_mesh_upload(frr_ctx *ctx, const float *vs_inputs, uint64_t ntris, int vs_id, int *mesh_out);
/* Same, data already in device memory (borrowed until frr_mesh_free). */
int frr_mesh_bind_device(frr_ctx *ctx, const void *dev_vs_inputs, uint64_t ntris, int vs_id, int *mesh_out);
/* The same mesh as a Model keeps it (obj_loader.rs; what init_vertex_input expands on the CPU, phong.rs:187-205): each
 * vertex once and three vertex numbers per triangle.
 * vertices: nverts x frr_vs_input_floats(vs_id) f32; indices: ntris x 3 u32, corner j of triangle t = vertices[indices[3t+j]]
 * == inputs[j] of phong.rs:190-197 with model.vert/uv/normal folded into one vertex record.
 * The mesh id is an ordinary one (frr_geometry, frr_draw, frr_readback_setup, frr_mesh_free ...), and everything a draw of
 * it produces -- images, triangle ids, emission order, statistics -- is that of the expanded mesh, bit for bit.
 * An index >= nverts is the reference's out-of-bounds panic (model.vert(i, j)): FRR_ERR_INVALID, no mesh id, and
 * frr_last_error names the first such triangle.  frr_mesh_upload_indexed checks on the host; frr_mesh_bind_device_indexed
 * with one small kernel over the index list on the ctx's stream and a host wait inside the call.  ntris == 0 is valid;
 * nverts == 0 with ntris > 0 is FRR_ERR_INVALID; ntris < 2^27 as above; device vertices 16-byte aligned, indices 4-byte.
 * Rewriting the vertices OR the indices of a device-bound mesh in place follows the rule of frr_create: frr_frame_fence,
 * rewrite, bind again -- and the new bind validates again.  (Should an index list be rewritten WITHOUT a re-bind, the
 * kernels still read only inside the vertex array: they clamp every index to nverts - 1.  That is a guard for the
 * machine, not a defined result.)  frr_debug_mvp does not take an indexed mesh (FRR_ERR_UNSUPPORTED). */
int frr_mesh_upload_indexed(frr_ctx *ctx, const float *vertices, uint64_t nverts,
                            const uint32_t *indices, uint64_t ntris, int vs_id, int *mesh_out);
int frr_mesh_bind_device_indexed(frr_ctx *ctx, const void *dev_vertices, uint64_t nverts,
                                 const void *dev_indices, uint64_t ntris, int vs_id, int *mesh_out);
int frr_mesh_free(frr_ctx *ctx, int mesh);
/* FrameBuffer used as texture (PSUniform.sample_2d_*, phong.rs:43-45): RGBA8 row-major.
 * height >= width is required: sample_2d clamps y with width (renderer.rs:523,525), so a
 * shorter texture is an out-of-bounds panic in the reference. */
int frr_texture_upload(frr_ctx *ctx, int slot, const uint8_t *rgba, uint32_t width, uint32_t height);
int frr_set_uniforms(frr_ctx *ctx, const frr_uniforms *u);
int frr_vs_input_floats(int vs_id);
int frr_vs_num_varyings(int vs_id);

/* ---- frame ------------------------------------------------------------------------------- */

/* frame_buffer.fill(rgba) + depth_buffer.fill(depth)  (phong.rs:316-317, renderer.rs:485-494).
 * Also resets the per-frame statistics and the setup list of a preceding frr_geometry.  The device
 * work is deferred: the next full-framebuffer frr_raster / frr_draw performs the clear inside its tile
 * kernel; every other call that can observe the targets or the statistics (frr_readback, frr_sync,
 * frr_get_stats, frr_target_ptrs, frr_bind_targets, a sub-window raster) settles it first, so the
 * observable behaviour is that of an immediate clear.  (Option clear_eager makes it immediate.)
 * `depth` may be any f32, NaN included: a fragment is rejected only where `rhw < depth` holds (renderer.rs:363), so a
 * NaN lets the first fragment of every pixel pass whatever its rhw, and stays where no fragment lands. */
int frr_clear(frr_ctx *ctx, const uint8_t rgba[4], float depth);

/* Loop A (phong.rs:321-331): Renderer::geometry_processing over every input triangle of `mesh`,
 * results concatenated in submission order on the device.  *ntris_setup (optional) forces a
 * stream sync to return the count. */
int frr_geometry(frr_ctx *ctx, int mesh, uint64_t *ntris_setup);
/* Loop B (phong.rs:361-381): Renderer::rasterization of the triangles of the last frr_geometry
 * with width_range=(x0,x1), height_range=(y0,y1) (renderer.rs:270-271).  As in the reference the
 * window is addressed locally: pixel (cx,cy) lands at colour (cx-x0, cy-y0) with row stride
 * `width` and at depth index (cy-y0)*x1 + (cx-x0) (renderer.rs:323,326,362,381).
 * With x0 < 0 the stride x1 is smaller than the window's width, so pixels of neighbouring rows share one depth entry; the
 * reference runs their fragments through it in submission order, and so does this library (one thread per entry instead
 * of the tile kernels: exact, and slow for large windows).  On a partitioned ctx the pixels of an entry may belong to
 * different ranks: the ranks' images of such a window do not stitch to the reference's. */
int frr_raster(frr_ctx *ctx, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1);
/* frr_geometry + frr_raster.  On a partitioned ctx (frr_set_partition, world > 1) the setup list frr_draw builds
 * keeps only the triangles that touch this rank's tile rows of THIS window: a later frr_raster with another
 * window, or after the partition changed, fails with FRR_ERR_INVALID (the reference may reuse one geometry for
 * several ranges, renderer.rs:269-271 -- call frr_geometry for that, it never filters), and so does
 * frr_readback_setup. */
int frr_draw(frr_ctx *ctx, int mesh, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1);

/* ---- instanced passes --------------------------------------------------------------------- */

/* One mesh under many model matrices in ONE geometry pass: the reference's loop over objects (phong.rs:319-331 runs
 * geometry_processing with a fresh vs_uniform.model per object) without one draw per object.
 * An instance table is ninst model matrices, 16 f32 each, column-major like frr_uniforms.model.
 * frr_geometry_instanced(mesh, inst) is BY DEFINITION this loop, concatenated into one setup list in that order:
 *     for i in 0..ninst:
 *         vs_uniform.model = models[i]                   (phong.rs:26-31, :119: mvp = proj * view * model)
 *         for t in 0..ntris: geometry_processing(mesh[t]) (renderer.rs:96-267)
 * and frr_draw_instanced is that loop followed by one Loop B over the list (renderer.rs:269-384).  Hence:
 * - Emission order is (instance, input triangle, fan triangle) (renderer.rs:245-266 within an input).  The id of a setup
 *   triangle of instance i is the frame's running count before the pass + what instances < i emitted + its offset
 *   within instance i; the ids of later draws of the frame continue behind the whole pass.  The ids of one instance are
 *   one contiguous range (ranged frr_shade_varyings: per-instance pixel uniforms).
 * - Where fragments tie in depth the later instance wins (renderer.rs:363: `rhw < depth` rejects, equal replaces), as
 *   the later triangle of one mesh does.
 * - Depth bits, ids, RGBA8, the setup list and tris_setup / frag_covered / frag_nan are, bit for bit, those of ninst
 *   plain frr_draw calls of the mesh, each after an frr_set_uniforms that differs only in model = models[i].
 * - Statistics: tris_in grows by ntris * ninst, draws by 1.
 * - Only the vertex shader sees the instance's matrices (the model matrix belongs to VSUniform, phong.rs:26-31;
 *   PSUniform, phong.rs:34-47, has none): in the geometry kernels u.mvp and u.model are the instance's, for built-in and
 *   user vertex shaders alike; every other field is the call's; the pixel shader sees the call's uniforms unchanged,
 *   u.model / u.mvp included.  A vertex shader that reads no matrix (FRR_VS_CLIP, FRR_VS_CLIP_COLOR) draws ninst
 *   identical copies, which is valid.
 * - mvp_i = (proj * view) * models[i] (phong.rs:119, left-associative), each product column by column as
 *   ((c0*x + c1*y) + c2*z) + c3*w with no contraction, computed on the device; frr_host_instance_mvp below is the host
 *   build of the same arithmetic.
 * - NaN, +-inf and all-zero matrices are not refused: the reference would compute with them.
 * ninst == 0 is a pass that emits nothing, like an empty mesh (draws still counts it); ninst == 1 is a plain draw under
 * models[0].  ntris * ninst >= 2^27: FRR_ERR_UNSUPPORTED (the order-key limit of the mesh entry points, on the product),
 * checked at the draw before anything is allocated.  FRR_ERR_INVALID: a NULL table with ninst > 0, a device pointer that
 * is not 16-byte aligned, an unknown or freed id.
 * A device-bound table is borrowed until frr_instances_free; rewriting it in place follows the rule of device-bound
 * meshes: frr_frame_fence, rewrite, bind again.  The call is logged, verified and replayed like frr_geometry / frr_draw,
 * and everything downstream of a geometry pass takes the instanced setup list as it is: frr_raster with any window,
 * frr_readback_setup, frr_draw_wireframe, frr_resolve_varyings, frr_shade_varyings, the partition filter of a draw. */
int frr_instances_upload(frr_ctx *ctx, const float *models, uint64_t ninst, int *inst_out);
int frr_instances_bind_device(frr_ctx *ctx, const void *dev_models, uint64_t ninst, int *inst_out);
int frr_instances_free(frr_ctx *ctx, int inst);
int frr_geometry_instanced(frr_ctx *ctx, int mesh, int inst, uint64_t *ntris_setup);
int frr_draw_instanced(frr_ctx *ctx, int mesh, int inst, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1);

/* ---- draw lists --------------------------------------------------------------------------- */

/* Many meshes, each under its own model matrix, in ONE geometry pass: the reference's whole setup loop (phong.rs:319-359
 * builds one setup list from three different meshes) as one call, and its rasterization loop (:361-381) as one tile kernel.
 * A draw list is nitems (mesh, model matrix) items; the matrix is 16 f32, column-major like frr_uniforms.model.
 * frr_geometry_list(list) is BY DEFINITION this loop, concatenated into one setup list in that order:
 *     for i in 0..nitems:
 *         vs_uniform.model = items[i].model
 *         for t in 0..ntris(mesh_i): geometry_processing(mesh_i[t])   (renderer.rs:96-267)
 * and frr_draw_list is that loop followed by one Loop B over the list (renderer.rs:269-384).  Hence:
 * - Depth bits, ids, RGBA8, the setup list and tris_setup / frag_covered / frag_nan are, bit for bit, those of nitems
 *   plain frr_draw calls of mesh_i, each after an frr_set_uniforms that differs only in model = items[i].model.
 * - Emission order is (item, input triangle, fan triangle).  The ids of one item are one contiguous range
 *   (frr_geometry_item_ranges below; ranged frr_shade_varyings: per-object pixel uniforms, the `place` rule of
 *   phong.rs:147-151); the ids of later draws of the frame continue behind the whole pass.  Where fragments tie in depth
 *   the later item wins (renderer.rs:363).
 * - Statistics: tris_in grows by the sum of the items' triangle counts, draws by 1.
 * - mvp_i = (proj * view) * items[i].model with the arithmetic of an instanced pass (frr_host_instance_mvp).  Only the
 *   vertex shader sees an item's matrices; the pixel shader runs with the call's uniforms.
 * - The cull mode of the call (frr_set_cull) is evaluated per (item, triangle) under that item's matrices.
 * - A list whose items all name one mesh is frr_draw_instanced of that mesh under the same matrices, bit for bit.
 * - Items may mix plain and indexed meshes, host-uploaded and device-bound ones; a device-bound mesh follows the rule
 *   for in-place rewrites unchanged (frr_frame_fence, rewrite, bind again -- and upload the list again: see below).
 * - All items must carry the same vs_id, built-in or user: otherwise the upload fails with FRR_ERR_INVALID and
 *   frr_last_error names the first offending item.
 * - nitems == 0 is a pass that emits nothing (draws still counts it); an item whose mesh has no triangles is valid at
 *   any position, several in a row too.  A list without items names no vertex shader: its pass has K = 0
 *   (frr_geometry_num_varyings), and there is nothing a pixel shader could fail to match -- frr_draw_list of it, and
 *   frr_raster behind frr_geometry_list of it, take any ps_id that names a shader (a built-in one, or a registered user
 *   shader of any K; FRR_PS_PHONG / FRR_PS_BLINN without a texture too) and draw nothing.
 * - The list is a SNAPSHOT taken at upload: the matrices, and per mesh its pointers, counts and registration.  Freeing a
 *   mesh that a live list names kills the list: frr_geometry_list / frr_draw_list of it return FRR_ERR_INVALID,
 *   frr_drawlist_free still takes it, and a later mesh that gets the freed id does not revive it.
 * - frr_debug_mvp is unaffected.
 * Errors: the sum of the items' triangle counts >= 2^27: FRR_ERR_UNSUPPORTED at upload, before anything is allocated;
 * reserved != 0, a NULL array with nitems > 0, an unknown or freed mesh or list id: FRR_ERR_INVALID.
 * The calls are logged, verified and replayed like frr_geometry / frr_draw (a replay fills the matrix table again and runs
 * under the cull mode and uniforms of the call), and everything downstream of a geometry pass takes the list's setup list
 * as it is: frr_raster with any window, frr_readback_setup, frr_draw_wireframe, frr_resolve_varyings,
 * frr_shade_varyings, the partition filter of a draw. */
typedef struct frr_draw_item { int32_t mesh; int32_t reserved; float model[16]; } frr_draw_item; /* reserved = 0 */
int frr_drawlist_upload(frr_ctx *ctx, const frr_draw_item *items, uint64_t nitems, int *list_out);
int frr_drawlist_free(frr_ctx *ctx, int list);
int frr_geometry_list(frr_ctx *ctx, int list, uint64_t *ntris_setup);
int frr_draw_list(frr_ctx *ctx, int list, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1);
/* Per item of the LATEST geometry pass: the frame-global emission index (= triangle id) of its first setup triangle, and
 * how many it emitted.  The items of a list pass, the instances of an instanced pass, one item for a plain pass.  An item
 * that emitted nothing has count 0 and first = where it would have started.  The numbers come from the pass's device
 * tables at the item boundaries (the setup list is not read back).  A synchronisation point like frr_readback_setup,
 * and FRR_ERR_INVALID where that fails: before any geometry pass, and after a frr_draw* that filtered the list on a
 * partitioned ctx.  With cap < *nitems it writes cap entries and still returns *nitems; either array may be NULL. */
int frr_geometry_item_ranges(frr_ctx *ctx, uint32_t *id_first, uint32_t *id_count, uint64_t cap, uint64_t *nitems);

/* Predicated list passes: keep or drop each item of a list by a value in device memory -- conditional rendering.
 * dev_keep_u32 is a caller-owned device buffer of one u32 per item.  THE KEEP RULE: item i is kept iff
 * keep[i] >= min_value, compared as unsigned; that one comparison is the whole rule.  With min_value = 1 the buffer is
 * exactly what frr_visible_pixels(FRR_PER_ITEM) wrote, or a 0/1 mask of 32-bit integers; a larger min_value skips what had
 * fewer than that many pixels; min_value = 0 keeps everything.  Entries at and beyond the list's item count are ignored.
 * A predicated list pass is BY DEFINITION frr_geometry_list / frr_draw_list over the same list with the mesh of every
 * dropped item replaced by an empty mesh.  Hence:
 * - The setup list, emission order, triangle ids, depth bits, RGBA8, tris_setup, frag_covered and frag_nan are those of
 *   that list, bit for bit -- the reference's loop over the kept items.  Ids stay dense over the survivors; the frame's
 *   running count continues behind them.
 * - The pass still has nitems items: frr_geometry_item_ranges reports every one, a dropped item with count 0 and first =
 *   where it would have started, and frr_visible_pixels(FRR_PER_ITEM) has nitems units with dropped items at 0 -- item k
 *   means the same object frame after frame, which is what lets a caller feed the counts back.
 * - tris_in grows by the list's FULL input count, dropped items included (the host does not know the mask; frr_set_cull
 *   counts the same way); draws by 1.  A dropped item's inputs emit nothing, like inputs with a w == 0: no fan slots, no
 *   clip-queue entries, no binning entries, no test against the partition -- and no vertex is loaded or shaded for them.
 * - The cull mode of the call still applies to the kept items, and everything downstream of a geometry pass takes the
 *   setup list as it is (see above).
 * Stream order: the buffer is read on the library's streams, once per execution of the pass, before the pass's geometry
 * kernel.  That read is ordered behind every command issued earlier on this ctx, whichever frame in flight or private
 * stream it ran on (the frr_visible_pixels of the previous frame that wrote the buffer is the intended producer), and
 * behind the streams of pending frr_frame_wait calls (a caller that wrote the mask on a stream of its own).  No host wait
 * is added for either.
 * Lifetime: the pass is logged and replayed like frr_geometry_list, and a replay reads the buffer again.  So the buffer
 * stays allocated until the next synchronisation point or frr_clear, and until then nobody but this ctx's own later
 * commands may change it (the rule of frr_shade_varyings' input).  A later frr_visible_pixels into the same buffer is
 * fine: a replay restarts at the failing command and runs in order.
 * Verification: what the pass needs of the work lists depends on data the host never sees, so it is never taken as proven
 * and proves nothing for any other call: the draw is verified inside the call every time, like a first pass.
 * Errors, FRR_ERR_INVALID: an unknown, freed or dead list, as frr_draw_list answers; keep_entries below the list's item
 * count; a NULL buffer with nitems > 0; a pointer that is not 4-byte aligned.  nitems == 0 is a valid pass that emits
 * nothing, and its buffer may be NULL.  Window and shader errors are those of frr_draw_list, in its order.  A refused
 * call leaves the ctx drawing. */
int frr_geometry_list_if(frr_ctx *ctx, int list, const void *dev_keep_u32, uint64_t keep_entries, uint32_t min_value,
                         uint64_t *ntris_setup);
int frr_draw_list_if(frr_ctx *ctx, int list, const void *dev_keep_u32, uint64_t keep_entries, uint32_t min_value, int ps_id,
                     int32_t x0, int32_t x1, int32_t y0, int32_t y1);

/* ---- face culling ------------------------------------------------------------------------- */

/* The reference draws every input triangle, whichever way it faces; frr_set_cull lets a geometry pass drop those that face
 * one way.  The reference destroys winding -- renderer.rs:205-218 sorts every triangle's vertices by angle around the
 * centroid, :309-312 swaps by orientation -- so facing cannot be read off the setup list: it is decided before the sort,
 * from the three clip positions (x, y, z, w) the vertex shader returned for the input, by the sign of the homogeneous
 * determinant
 *     d = (x0*(y1*w2 - y2*w1) - x1*(y0*w2 - y2*w0)) + x2*(y0*w1 - y1*w0)
 * in f32 with exactly this association and no contraction (frr_host_cull_det below is the host build of the device's
 * code).  With all w > 0, d > 0 means vertices 0, 1, 2 run counter-clockwise in NDC (x right, y up), i.e. clockwise on
 * the displayed image, whose y runs down; for a triangle that crosses w = 0 the sign is still a defined rule, which is
 * why the determinant is used and not a screen-space area.  The rule is the f32 formula BY DEFINITION, not the exact sign:
 * for near-degenerate triangles the two differ often.  FRR_CULL_NEG drops inputs with d < 0, FRR_CULL_POS those with
 * d > 0; d == 0 and a NaN d are never dropped (both comparisons are false, and the reference would compute with such
 * triangles).  The modes are named by sign, not front / back, because meshes differ in winding.
 * A geometry pass under a cull mode is BY DEFINITION the plain pass over the sub-mesh of the inputs the mode keeps, in
 * their original order.  Hence:
 * - The setup list, emission order, triangle ids, depth bits, RGBA8, tris_setup, frag_covered and frag_nan are, bit for
 *   bit, those of drawing that sub-mesh with FRR_CULL_NONE.  Ids stay dense over the survivors, and the frame's running
 *   count continues behind them.
 * - tris_in still grows by the number of inputs submitted, culled ones included; draws is as before.
 * - The pos.w == 0.0 rule (geometry_processing returns None, renderer.rs:117-119) comes first and is unchanged; a culled
 *   input is one more input that emits nothing.  One that would have been clipped gets no fan slots.
 * - The determinant is taken on what the vertex shader returned: built-in or user vertex shaders, plain or indexed meshes
 *   alike; in an instanced pass it is evaluated per (instance, triangle) under that instance's matrices (a mirrored
 *   instance faces the other way).
 * - Everything that consumes a setup list takes the culled one as it is: frr_raster with any window, frr_readback_setup,
 *   frr_draw_wireframe (no edges for culled inputs), frr_resolve_varyings, ranged frr_shade_varyings, the partition
 *   filter of frr_draw.
 * - The culled frame is NOT in general the unculled frame, not even for a closed mesh: at a silhouette a back face can own
 *   a pixel no front face covers (at 240 x 135: 34 depth entries / 12 colour pixels of the project's torus scene, 2 / 2 of
 *   its sphere scene).
 * frr_set_cull applies to the geometry passes issued from now on (frr_geometry, frr_draw and the _instanced pair); the
 * mode travels with each pass like frr_uniforms, so a replayed pass runs under the mode of its call, and frr_clear does
 * not reset it.  frr_raster after frr_geometry rasterizes the list as it was built, whatever the mode is by then.
 * An unknown mode is FRR_ERR_INVALID and changes nothing. */
int frr_set_cull(frr_ctx *ctx, int mode);

/* ---- lines ------------------------------------------------------------------------------- */

/* FrameBuffer::draw_line(x1, y1, x2, y2, color) (renderer.rs:540-588), the reference's only drawing primitive besides the
 * triangle, for a whole list of calls at once.  Everything the reference does is reproduced: the endpoints are sorted per
 * axis, independently (:541-542: a falling line is drawn as the rising one), a vertical or horizontal line excludes its upper
 * end (:548, :553), every other line paints a second pixel in the column (row) where its minor coordinate steps and ends
 * with (x2, y2) (:563-572, :575-584), and set_pixel addresses linearly with no test of x (:497-503): x >= width lands in a
 * later row.
 * A list is nlines x {x1, y1, x2, y2} u32 and nlines x RGBA8, in call order.  A segment for which the reference would panic
 * -- the largest linear pixel index of its walk, computed in 64 bits, is >= width * height of the ctx -- makes the whole list
 * FRR_ERR_INVALID: no list id, and frr_last_error names the first such segment.  frr_lines_upload checks on the host;
 * frr_lines_bind_device (borrowed device memory, xyxy 16-byte and rgba 4-byte aligned) with one small kernel on the ctx's
 * stream and a host wait inside the call.  nlines == 0 is valid; nlines < 2^31.  Rewriting a device-bound list in place
 * follows the rule of frr_create for device-bound meshes: frr_frame_fence, rewrite, bind again -- and the new bind validates
 * again.  (Should a list be rewritten WITHOUT a re-bind, the kernels still write only inside the colour target: a segment
 * or a pixel that would leave it is dropped.  That is a guard for the machine, not a defined result.) */
int frr_lines_upload(frr_ctx *ctx, const uint32_t *xyxy, const uint8_t *rgba, uint64_t nlines, int *lines_out);
int frr_lines_bind_device(frr_ctx *ctx, const void *dev_xyxy, const void *dev_rgba, uint64_t nlines, int *lines_out);
int frr_lines_free(frr_ctx *ctx, int lines);
/* for k in 0..nlines: frame_buffer.draw_line(x1[k], y1[k], x2[k], y2[k], rgba[k]) on the ctx's colour target (row stride =
 * the ctx's width).  Colour only: depth and triangle ids are untouched, and so is every field of frr_stats.  The call is
 * ordered like any command that writes the targets -- behind the draws issued before it and before those issued after it: a
 * later triangle draw overwrites a line pixel wherever its fragment passes the depth test, and nowhere else -- and where
 * segments of the list meet, the later one's colour stays.  A pending frr_clear is settled first, as by a sub-window
 * raster.  On a partitioned ctx a pixel is written only if this rank owns the tile row of its linear index
 * ((index / width) / 32) among the tile rows of the CTX, so that the ranks' images stitch to the reference's like those of any
 * draw -- of any draw whose window has as many tile rows as the ctx, or in the interleaved layout.  A draw takes its owner from
 * the tile rows of its WINDOW (frr_set_partition_layout), and in the blocked layout a shorter window divides other rows: on a
 * 96-row ctx a window of 40 rows has two tile rows, and with two ranks plane rows 32 .. 39 are the draws' on rank 1 and the
 * lines' on rank 0, so a line over a triangle there is complete on no rank.  Use the interleaved layout, or full-height
 * windows, where lines and draws meet. */
int frr_draw_lines(frr_ctx *ctx, int lines);
/* The edges (v0,v1), (v1,v2), (v2,v0) of every triangle of the last frr_geometry in one colour: segment 3t + e is edge e of
 * setup triangle t, between the spi of its emission-order vertices (what frr_readback_setup returns).  The reference has no
 * caller of draw_line to copy, so this rule is the library's own: an edge with an endpoint outside 0 <= x < width,
 * 0 <= y < height is skipped whole.  The result is by definition that of frr_draw_lines on the list a host would build that
 * way from frr_readback_setup -- without the read-back: the triangle count is taken from the device tables, and the call
 * waits for nothing on the host.  It fails where frr_readback_setup fails (FRR_ERR_INVALID after a frr_draw that filtered
 * the setup list on a partitioned ctx). */
int frr_draw_wireframe(frr_ctx *ctx, const uint8_t rgba[4]);

/* ---- the pixel shader's input as a buffer (deferred shading) -------------------------------- */
/* The ShaderContext the reference hands to the pixel shader -- `input` of renderer.rs:368-378, the perspective-correct
 * interpolation of the winning triangle's varyings -- for every pixel of a window, pixel-major f32 [entries][K].
 *   K       the varyings of the latest frr_geometry / frr_draw, frr_vs_num_varyings of its vs_id (user shaders included, up
 *           to FRR_MAX_VARYINGS).
 *   window  (x0, x1) x (y0, y1): the one the raster passes of that geometry used.  Pixel (cx, cy) has the depth index
 *           i = (cy - y0) * x1 + (cx - x0) (renderer.rs:362).
 * Where the triangle-id target at i names a triangle of the latest geometry pass (tri_base <= id < tri_base + its triangle
 * count), out[i * K + k], k < K, becomes i0 * c0 + i1 * c1 + i2 * c2 of renderer.rs:374-378 for that triangle at that
 * pixel, from the barycentrics of :343-360 and w, c0, c1, c2 of :368-372 -- the arithmetic and association of the tile
 * kernel's resolve (1 / (rhw != 0 ? rhw : 1), r * a * w, no contraction), so the value is the very one the built-in and user
 * pixel shaders receive.  EVERY OTHER ENTRY OF out IS LEFT UNTOUCHED: a frame of several draws composes -- called after each
 * draw, the buffer ends with every pixel holding the varyings of its final owner (K may differ between the draws only if
 * the caller keeps a buffer per K).  Which pixel shader the raster pass ran does not matter: after a FRR_PS_DEPTH draw the
 * result is the same.
 * frr_resolve_varyings: dev_out_f32 is device memory, 4-byte aligned, of out_entries * K floats; rows whose addresses allow
 * it leave as 16-byte stores.  It is a command like a wireframe: it runs on the current frame's stream behind the draws
 * issued so far and before those issued after it, settles a pending frr_clear first (as a sub-window raster does), reads the
 * current frame's target set (own or caller-bound) and the geometry pass's tables on the device, and waits for nothing on
 * the host.  The caller orders its reads of dev_out_f32 with frr_frame_fence or frr_sync, as for bound targets -- with
 * frr_frame_fence on a stream of its own: a NULL stream there means the ctx's stream, so the legacy default stream (handle
 * 0, what torch uses unless told otherwise) cannot be fenced; read on a created stream, or after frr_sync.  Behind a
 * command that found a work list too small it writes nothing and is replayed with that command -- so dev_out_f32 stays
 * allocated until the next synchronisation point or frr_clear, like a bound target.  frr_clear forgets the commands
 * logged so far: a resolve that was cancelled by a failure the host has not seen by then is not replayed (the frame's
 * targets are overwritten by the clear, the caller's buffer keeps what it held).  A draw verifies itself before it returns
 * (frr_frame_fence), so a resolve issued after the frr_raster / frr_draw of its geometry pass is never cancelled; one issued
 * between frr_geometry and frr_raster is guaranteed only once a synchronisation point has passed before the next
 * frr_clear.  On a partitioned ctx only the pixels
 * of the window's tile rows this rank owns are written.
 * frr_readback_varyings: the same into host memory -- a temporary device buffer starts as a copy of host_inout, the
 * command runs, and after a synchronisation point the buffer is copied back: "untouched" holds on the host too.
 * Errors.  FRR_ERR_INVALID: out_entries < (y1 - y0) * x1; x1 <= x0, y1 <= y0 or a window beyond what frr_raster accepts;
 * a NULL or misaligned buffer; a call before any frr_geometry; a setup list filtered by frr_draw on a partitioned ctx (where
 * frr_draw_wireframe and frr_readback_setup fail: use frr_geometry + frr_raster).  FRR_ERR_UNSUPPORTED: x0 < 0 -- pixels of
 * neighbouring rows share depth entries there, so an entry has no single pixel.  K == 0, an empty mesh, or a frr_clear since
 * the geometry pass: FRR_OK, nothing written. */
/* K of the latest frr_geometry / frr_draw (what sizes the buffers above); FRR_ERR_INVALID before any geometry pass */
int frr_geometry_num_varyings(const frr_ctx *ctx);
int frr_resolve_varyings(frr_ctx *ctx, int32_t x0, int32_t x1, int32_t y0, int32_t y1, void *dev_out_f32, uint64_t out_entries);
int frr_readback_varyings(frr_ctx *ctx, int32_t x0, int32_t x1, int32_t y0, int32_t y1, float *host_inout, uint64_t out_entries);

/* ---- shading a varyings buffer (the other half of deferred shading) ------------------------- */
/* The step from the pixel shader's input to the colour target -- renderer.rs:380-381 with vec4_to_u8_array (:7-14) and
 * set_pixel (:497-503) -- over a buffer of varyings, pixel-major f32 [in_entries][K]: what frr_resolve_varyings wrote, or
 * anything the caller made.
 *   window  (x0, x1) x (y0, y1).  Pixel (cx, cy) has the depth index i = (cy - y0) * x1 + (cx - x0) (renderer.rs:362).
 *   id      the current frame's triangle-id target at i: the frame-global emission index of the pixel's owner, 0xFFFFFFFF
 *           where nothing was drawn.
 * The pixel is shaded where id != 0xFFFFFFFF and id - id_first < id_count (unsigned).  A shaded pixel's colour, at
 * (cx - x0, cy - y0) with row stride = the ctx's width -- exactly where frr_raster writes it -- becomes
 * vec4_to_u8_array(pixel_shader(uniforms, &in[i * K])): the shader and the quantisation of the tile kernel's resolve, the
 * same functions with no contraction, so a FRR_PS_DEPTH draw + frr_resolve_varyings + frr_shade_varyings leaves the colour
 * of the forward draw bit for bit.  EVERY OTHER COLOUR PIXEL IS LEFT UNTOUCHED, and so are depth, triangle ids and every
 * field of frr_stats.  id_first = 0, id_count = 0xFFFFFFFF: every drawn pixel; id_count = 0: FRR_OK, nothing written.
 * Ranges of ids are how one G-buffer takes pixel uniforms per range of triangles: set the uniforms, shade a range, set
 * others, shade the next (phong.rs:361-370 as three calls).
 * It needs no geometry pass: it reads only the buffer, the id target and the uniforms, so it also works after a frr_draw
 * that filtered the setup list on a partitioned ctx, and after a frr_clear (nothing is drawn: nothing is written).
 * Uniforms: textures, frr_set_uniforms and frr_set_user_uniforms as of the call travel with the command, as with a draw; a
 * replay shades with the uniforms of the original call.
 * ps_id and K follow the rule frr_raster applies between a pixel shader and its geometry's K: FRR_PS_COLOR needs K = 3,
 * FRR_PS_PHONG / FRR_PS_BLINN K = 8 and a texture in uniforms.texture_slot, a user id the K it was registered with;
 * FRR_PS_FLAT takes any 0 <= K <= FRR_MAX_VARYINGS (with K == 0 the buffer may be NULL); FRR_PS_DEPTH has nothing to shade.
 * frr_shade_varyings: dev_in_f32 is device memory, 4-byte aligned; where K is a multiple of 4 and the buffer 16-byte
 * aligned the entries are read with 16-byte loads.  It is a command that writes a target, like frr_draw_lines: it runs on
 * the current frame's stream behind the draws, resolves and lines issued before it and before those issued after it,
 * settles a pending frr_clear first, waits for the streams of pending frr_frame_wait calls (how a caller who filled the
 * buffer on a stream of its own orders that write before the shade), uses the current target set (own or caller-bound, one
 * or two frames in flight) and waits for nothing on the host.  Behind a command that found a work list too small it writes
 * nothing and is replayed with that command, so THE BUFFER MUST STAY ALLOCATED AND UNCHANGED until the next
 * synchronisation point or frr_clear, like the output of frr_resolve_varyings.  On a partitioned ctx only the pixels of
 * the window's tile rows this rank owns are written.
 * frr_shade_varyings_host: the same from host memory -- the first (y1 - y0) * x1 entries of host_in are copied into a
 * temporary device buffer (the call returns when the copy is done: host_in may be reused at once) that the ctx keeps
 * until the next synchronisation point or frr_clear, where a replay still finds it.
 * Errors.  FRR_ERR_INVALID: in_entries < (y1 - y0) * x1; x1 <= x0, y1 <= y0 or a window beyond what frr_raster accepts; a
 * NULL buffer (with K > 0) or one not 4-byte aligned; a ps_id or K the rule above refuses.  FRR_ERR_UNSUPPORTED: x0 < 0 --
 * as for frr_resolve_varyings, an entry has no single pixel there. */
int frr_shade_varyings(frr_ctx *ctx, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                       const void *dev_in_f32, uint64_t in_entries, int K,
                       uint32_t id_first, uint32_t id_count);
int frr_shade_varyings_host(frr_ctx *ctx, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                            const float *host_in, uint64_t in_entries, int K,
                            uint32_t id_first, uint32_t id_count);

/* ---- per-item materials: one shade for all the items of a pass --------------------------------- */
/* The reference gives every object its own ps_uniform.place, and so its own texture, inside one frame (phong.rs:34-47,
 * 361-370).  A material is that for a list: the pixel uniforms that change from item to item, 64 bytes each, in a table on
 * the device with one entry per item of a geometry pass.
 * The items are those of the LATEST geometry pass, exactly the ones frr_geometry_item_ranges reports (id_first[k],
 * id_count[k], nitems): the items of a list pass, the instances of an instanced pass, one item for a plain pass.
 * frr_shade_items(ps_id, window, buffer, in_entries, K, materials) is BY DEFINITION this loop, in this order:
 *   for k in 0 .. nitems:
 *       u = the uniforms of the call, with uniforms.texture_slot (hence the texture frr::sample_2d and FRR_PS_PHONG /
 *           FRR_PS_BLINN read), ambient_strength, specular_strength, flat_color and u.user[0 .. FRR_MATERIAL_USER) taken
 *           from materials[k]
 *       frr_shade_varyings(ps_id, window, buffer, in_entries, K, id_first[k], id_count[k])   under u
 * so that:
 * - the colour target is, byte for byte, what that loop of calls leaves: the same pixel shader and quantisation under the
 *   same uniform values;
 * - pixels whose id is not one of the latest pass's (nothing drawn, earlier passes of the frame) are untouched, and so are
 *   depth, triangle ids and every field of frr_stats;
 * - everything else in the uniforms is the call's: view_pos, light_pos, light_color, u.user[FRR_MATERIAL_USER ..), every
 *   texture slot (frr::sample_2d_slot), and u.model / u.mvp, which a pixel shader sees as under frr_shade_varyings;
 * - it is ordered, logged and replayed as frr_shade_varyings is -- a command that writes a target on the current frame's
 *   stream, behind a pending frr_clear and the streams of pending frr_frame_wait calls, with no host wait, on a partitioned
 *   ctx writing only the tile rows this rank owns -- AND as frr_visible_pixels is against the pass: behind the pass's
 *   geometry, whose tables it reads on the device.  A replay shades with the uniforms of the call and reads the table again;
 * - THE BUFFER, AND A DEVICE-BOUND TABLE, MUST STAY ALLOCATED AND UNCHANGED until the next synchronisation point or
 *   frr_clear.
 * An item's material covers exactly the item's ids.  The reference's loop switches its uniform at `i <= body_offset`
 * (phong.rs:364-369), one triangle late; this command does NOT reproduce that off-by-one -- the ranged frr_shade_varyings
 * calls of INTEGRATION.md section 1d stay the way to.
 * Tables.  frr_materials_upload copies n materials (the host checks them); frr_materials_bind_device borrows device memory,
 * 16-byte aligned, until frr_materials_free, and checks it with one small kernel on the ctx's stream and a host wait inside
 * the call, as frr_lines_bind_device does (after an in-place rewrite: frr_frame_fence, rewrite, bind again).  A material with
 * a texture_slot outside 0 .. FRR_MAX_TEXTURES-1 or with reserved != 0 is refused with FRR_ERR_INVALID, and frr_last_error
 * names the first such entry; NaN and infinite values are the caller's business.  (The kernel clamps the slot anyway: a
 * guard for the machine, not a defined result.)  n == 0 is a valid table.  frr_materials_free finishes what is in flight
 * first, as frr_instances_free does.
 * Errors of frr_shade_items, in this order.  The window, shader and buffer rules of frr_shade_varyings (the texture of a
 * lit shader is asked of the table, below).  FRR_ERR_INVALID: an unknown or freed table id; a call before any geometry
 * pass, or after a frr_draw* that filtered the setup list on a partitioned ctx (where frr_visible_pixels fails); a table
 * with fewer entries than the pass has items (more are fine: the rest is ignored); with FRR_PS_PHONG / FRR_PS_BLINN, a slot
 * some entry of the table names that holds no texture at the call (frr_last_error names the slot) -- for a user pixel
 * shader an empty slot samples as zero: frr::sample_2d_slot as ever, and frr::sample_2d(u, ...) -- the material's own slot --
 * because a material that names an empty slot is given a 1 x 1 texture of zeros (zero at every finite coordinate; a NaN or
 * infinite coordinate gives NaN there as on any texture).  Under frr_shade_varyings frr::sample_2d of an empty
 * uniforms.texture_slot stays undefined, as before.  After a frr_clear since the pass, for a pass without inputs and for nitems == 0:
 * FRR_OK, nothing written.
 * frr_shade_items_host: the buffer from host memory, as frr_shade_varyings_host takes it. */
#define FRR_MATERIAL_USER 8
typedef struct frr_material {          /* 64 bytes: four 16-byte loads */
    int32_t texture_slot;              /* PSUniform.place, 0 .. FRR_MAX_TEXTURES-1 */
    float   ambient_strength, specular_strength;
    int32_t reserved;                  /* 0 */
    float   flat_color[4];
    float   user[FRR_MATERIAL_USER];   /* replaces u.user[0 .. FRR_MATERIAL_USER) */
} frr_material;
int frr_materials_upload(frr_ctx *ctx, const frr_material *mats, uint64_t n, int *materials_out);
int frr_materials_bind_device(frr_ctx *ctx, const void *dev_mats, uint64_t n, int *materials_out);
int frr_materials_free(frr_ctx *ctx, int materials);
int frr_shade_items(frr_ctx *ctx, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                    const void *dev_in_f32, uint64_t in_entries, int K, int materials);
int frr_shade_items_host(frr_ctx *ctx, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                         const float *host_in, uint64_t in_entries, int K, int materials);

/* ---- visible pixel counts --------------------------------------------------------------------- */
/* Which objects of a pass ended up on screen, and with how many pixels, without reading the frame back: the triangle-id
 * target of a window as counts, on the device.  (The reference has no such query; every renderer with a batched draw has:
 * occlusion queries, picking, choosing a level of detail, visible-triangle sets for baking.)
 *   window  (x0, x1) x (y0, y1), addressed as everywhere else: pixel (cx, cy) has the depth index
 *           i = (cy - y0) * x1 + (cx - x0) (renderer.rs:362).  The entries of the window are those i with
 *           0 <= cx - x0 < x1 - x0 and 0 <= cy - y0 < y1 - y0.
 *   id      id[i]: the current frame's triangle-id target at the command's place in the stream.
 * FRR_PER_ITEM      The units are the items of the LATEST geometry pass, exactly the ones frr_geometry_item_ranges reports:
 *                   the items of a list pass, the instances of an instanced pass, one item for a plain pass.  out[k] = the
 *                   number of window entries with id[i] != 0xFFFFFFFF and id[i] - id_first[k] < id_count[k] (unsigned), with
 *                   id_first and id_count as frr_geometry_item_ranges would return them.  Pixels owned by earlier passes of
 *                   the frame count for nobody.
 * FRR_PER_TRIANGLE  The units are the frame-global emission indices 0 .. T, T = the frame's running triangle count behind
 *                   the latest geometry pass (its first id plus what it emitted).  out[t] = the number of window entries with
 *                   id[i] == t.  This covers every pass of the frame so far: a caller who wants per-item counts over several
 *                   passes sums the ranges it got from frr_geometry_item_ranges after each pass.
 * With n units, EVERY one of the out_entries entries is written: unit k < min(n, out_entries) gets its count, entries at and
 * beyond n get 0; a unit >= out_entries is counted nowhere.  Colour, depth, ids and every field of frr_stats are untouched.
 * The counts are sums of integers: two runs give the same bytes.
 * After a frr_clear since the geometry pass the id target holds nothing of it: FRR_OK, all zeros; n is still the pass's item
 * count for FRR_PER_ITEM, and 0 for FRR_PER_TRIANGLE.  An empty list, an empty mesh, ninst == 0 and items that emit nothing
 * are valid and count 0.
 * frr_visible_pixels: dev_out_u32 is device memory, 4-byte aligned, of out_entries u32.  It is a command like
 * frr_resolve_varyings: it runs on the current frame's stream behind the draws issued so far and before those issued after
 * it -- a later draw that occludes an item does not change a count queued before it --, settles a pending frr_clear first,
 * reads the current target set (own or caller-bound, one or two frames in flight) and the pass's tables on the device, and
 * waits for nothing on the host.  The caller orders its reads of dev_out_u32 with frr_frame_fence (on a created stream, see
 * frr_resolve_varyings) or frr_sync.  It is logged and replayed: behind a command that found a work list too small it writes
 * nothing, not even the zeros, and is replayed with that command -- so dev_out_u32 stays allocated until the next
 * synchronisation point or frr_clear.
 * On a partitioned ctx only entries in tile rows this rank owns are counted, so the ranks' counts add up to the unpartitioned
 * ones; after a frr_draw* that filtered the setup list the call fails with FRR_ERR_INVALID, where
 * frr_geometry_item_ranges fails.
 * frr_visible_pixels_host: the same through a temporary device buffer into host memory; a synchronisation point.  *nunits
 * (optional) receives n.
 * Errors.  The window rules of frr_resolve_varyings: FRR_ERR_UNSUPPORTED for x0 < 0; FRR_ERR_INVALID for x1 <= x0, y1 <= y0, a
 * window larger than the FrameBuffer, coordinates outside the i16 range, a depth index that leaves the buffer.
 * FRR_ERR_INVALID also: an unknown unit, a NULL or not 4-byte-aligned buffer with out_entries > 0, a call before any geometry
 * pass.  out_entries == 0 (after these checks): FRR_OK, and nothing happens (*nunits is not written either). */
typedef enum frr_visible_unit { FRR_PER_ITEM = 0, FRR_PER_TRIANGLE = 1 } frr_visible_unit;
int frr_visible_pixels(frr_ctx *ctx, int unit, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                       void *dev_out_u32, uint64_t out_entries);
int frr_visible_pixels_host(frr_ctx *ctx, int unit, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                            uint32_t *host_out, uint64_t out_entries, uint64_t *nunits);

/* ---- occlusion queries ------------------------------------------------------------------------- */
/* Would the triangles of a pass be visible against the depth that is there now?  Loop B (renderer.rs:269-384) over the
 * triangles of the LATEST geometry pass with every store taken out: the fragments that pass the depth test are counted,
 * nothing is drawn.  (frr_visible_pixels counts what a draw left behind; this asks before anything is drawn -- of a cheap
 * proxy of an object, or of the object itself -- and its counts are a keep buffer for frr_draw_list_if.)
 *   fragment  Setup triangle t of the pass has a fragment at pixel (cx, cy) of the window under exactly the conditions of the
 *             reference, and of frr_raster of the same pass in the same window: inside the triangle's box clamped to the
 *             window (:285-298), accepted by the three wrapping-i32 edge tests with the top-left rule (:329-341), and
 *             a + b + c != 0 (:351-354).
 *   test      The fragment passes iff `rhw < depth[i]` is false (:363), i = (cy - y0) * x1 + (cx - x0), rhw that of :360 in the
 *             tile kernel's arithmetic, depth[i] the current frame's depth target at the command's place in the stream.  A
 *             NaN rhw passes, a NaN depth lets everything pass, rhw == depth passes.
 * The query's own fragments store nothing, so EVERY fragment meets the same stored value -- unlike the reference's loop, where
 * an earlier triangle of the pass raises the depth for a later one.  Said the other way round: the count of triangle t is the
 * number of entries rasterization(t) ALONE changes on a copy of the depth buffer.
 * Units, n and the every-entry-is-written rule are frr_visible_pixels': FRR_PER_ITEM out[k] = the sum over the triangles of
 * item k of the latest pass (the items frr_geometry_item_ranges reports); FRR_PER_TRIANGLE out[e] for the frame-global
 * emission index e, indices below the pass's first id get 0.  Unit k < min(n, out_entries) gets its count, entries at and
 * beyond n get 0, a unit >= out_entries is counted nowhere.
 * Colour, depth and ids are untouched, and so is every field of frr_stats (frag_covered and frag_nan are not counted) except
 * `replays`, where a replay happens.  The counts are sums of integers: two runs give the same bytes.
 * frr_query_pixels: a command on the current frame's stream like frr_visible_pixels: behind the draws issued so far and in
 * front of those issued after it; it settles a pending frr_clear first (and is never fused with it), reads the current target
 * set (own or caller-bound, one or two frames in flight) and waits for nothing on the host beyond what frr_raster waits for.
 * The caller orders its own reads of dev_out_u32 with frr_frame_fence or frr_sync; a later frr_draw_list_if / frr_geometry_list_if
 * of this ctx that names the buffer is already ordered behind it (the keep buffer is read behind every command issued on the
 * ctx so far).
 * Work lists.  The query bins its triangles exactly as frr_raster of the same pass in the same window does: it is logged,
 * verified inside the call and replayed by frr_raster's rules, and shares the proof of that raster signature (a pass behind a
 * *_list_if geometry is never taken as proven).  A replay zeroes and counts again; behind a failed command the query writes
 * nothing, not even the zeros, so dev_out_u32 stays allocated until the next synchronisation point or frr_clear.  It closes
 * an open pass in the sense of the frr_frame_fence comment.
 * frr_geometry*; frr_query_pixels; frr_raster on one pass is valid: the raster draws what frr_draw* would have drawn.  A pass
 * that is only queried is an ordinary geometry pass that nothing rasterized (its ids, tris_in and tris_setup are taken).
 * On a partitioned ctx only the tile rows this rank owns are counted, so the ranks' counts add up to the unpartitioned ones;
 * after a frr_draw* that filtered the setup list the call fails with FRR_ERR_INVALID, where frr_visible_pixels fails.
 * After a frr_clear since the pass, for an empty pass and for a pass without items: FRR_OK and zeros.
 * Option "visible_lds_bins" is this command's test hook too: per item, more units than v add to global memory directly
 * instead of through the LDS histogram (per triangle the adds always go to global memory, one per tile and triangle).
 * frr_query_pixels_host: the same through a temporary device buffer into host memory; a synchronisation point.  *nunits
 * (optional) receives n.
 * Errors: those of frr_visible_pixels -- FRR_ERR_UNSUPPORTED for x0 < 0 (one triangle could hit an entry twice), FRR_ERR_INVALID
 * for the other window rules, an unknown unit, a NULL or not 4-byte-aligned buffer with out_entries > 0, a call before any
 * geometry pass.  A refused call leaves the ctx drawing.  out_entries == 0 (after these checks): FRR_OK, nothing happens. */
int frr_query_pixels(frr_ctx *ctx, int unit, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                     void *dev_out_u32, uint64_t out_entries);
int frr_query_pixels_host(frr_ctx *ctx, int unit, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                          uint32_t *host_out, uint64_t out_entries, uint64_t *nunits);
/* host build of the query's depth test (cf. frr_host_list_item): 1 iff a fragment of that rhw passes against that depth */
int frr_host_fragment_passes(float rhw, float depth);

/* ---- box queries ------------------------------------------------------------------------------- */
/* The cheap occlusion test: per item of a draw list the object-space box of its mesh, projected under the item's own matrix,
 * against the farthest depth stored under its screen rectangle.  No geometry pass, no binning, no work list, no host wait.
 * The test is conservative: out[i] == 0 implies that drawing item i now changes no entry of colour, depth or ids, and out[i]
 * is an upper bound of what frr_visible_pixels(FRR_PER_ITEM) can report for the item after it is drawn now -- so the buffer is
 * a keep buffer for frr_draw_list_if (min_value 1), and with a larger min_value contribution culling before anything is drawn.
 * It is not exact: an item it keeps may still own no pixel (frr_query_pixels of the item's own mesh answers that).
 *
 * frr_drawlist_bounds: per item the object-space AABB lo, hi of the positions (floats 0..2 of a vertex record) of the corners
 * its triangles name -- for an indexed mesh the corners gathered through the indices, clamped as the geometry kernels clamp,
 * so an unreferenced vertex does not widen the box -- and flags: bit 0, some referenced component is NaN or +-inf (lo / hi are
 * then unspecified); bit 1, the mesh has no triangles (lo / hi are zeros).  -0.0 is reported as +0.0.  Computed on the device,
 * once per distinct mesh of the list's snapshot, in integer atomics only (two runs give the same bytes); on the ctx's stream
 * behind what it holds, and the call waits for it on the host (a set-up call and a synchronisation point, like
 * frr_mesh_bind_device_indexed's check).  The table stays with the list until frr_drawlist_free; a second call computes it
 * again (after an in-place rewrite of a device-bound mesh: fence, rewrite, bind again, upload the list again, then this).
 * host_lo_hi ([cap][6]: lo xyz, hi xyz) and host_flags ([cap]) receive min(cap, n) items where not NULL; *nitems receives n.
 * Errors: FRR_ERR_INVALID for an unknown, freed or dead list; FRR_ERR_UNSUPPORTED, and no table is stored, where the list's
 * vertex shader is not FRR_VS_PHONG or FRR_VS_GOURAUD -- the inputs of FRR_VS_CLIP* are clip coordinates, there is no object
 * space, and a user vertex shader may move a vertex anywhere, so a box of its inputs bounds nothing.  A list without items is
 * valid whatever its shader.
 *
 * frr_query_boxes: for item i with lo, hi, flags and mvp_i = (proj * view) * items[i].model (the arithmetic of
 * frr_host_instance_mvp: the bits the list pass transforms the item with; proj, view the uniforms of the call; the viewport is
 * the ctx's W, H), in f32 with the written association (f_renderer_amd/csrc/frr_boxes.h is the definition):
 *   NONE       flag bit 1: out = 0.
 *   corners    corner j = 0..7 (bit k of j picks hi[k]): clip_j = mvp_i * (c, 1), rhw, ndc, spf, spi by renderer.rs:223-234.
 *   E          = |mvp_i| * (a, 1) * 2^-21, a = max(|lo|, |hi|) per axis: twice the rounding error of any vertex's clip position.
 *   UNBOUNDED  flag bit 0; a clip component, an ndc or E not finite; a corner with z_j - E_z < 0 (the reference's near-plane
 *              intersection, renderer.rs:70, leaves the triangle) or w_j - E_w <= 0; wmin - 2 E_w <= 0; a guard of 2^15 or
 *              more.  out = the window's pixels.
 *   rectangle  [min spi.x - Gx, max spi.x + Gx) x [min spi.y - Gy, max spi.y + Gy) clamped to the window; G = 1 + (int)d,
 *              d = eps * D + (n + 1) * D * 2^-21, eps = (E_axis + n * E_w) / (wmin - 2 E_w) + n * 2^-21, n the corners' largest
 *              |ndc| on the axis and D = W or H.  Empty: OUTSIDE, out = 0.
 *   zub        = (1 / (wmin - E_w)) * (1 + 2^-18): no fragment of the item has a larger rhw.
 *   region     in window-local coordinates the smallest level s >= 2 at which the rectangle touches at most 4 x 4 cells of
 *              2^s x 2^s pixels; dmin = the smallest depth key (a NaN depth below everything) over those cells cut to the window,
 *              depth[(cy - y0) * x1 + (cx - x0)] (renderer.rs:362).
 *   verdict    HIDDEN iff key(zub) < dmin, strictly (a tie keeps, as the depth test lets ties pass): out = 0; else KEPT: out =
 *              the pixels of the clamped rectangle.
 * Units: n = the list's items; unit k < min(n, out_entries) gets its value, entries at and beyond n get 0, a unit >=
 * out_entries is written nowhere.  A command on the current frame's stream like frr_visible_pixels: behind the draws issued
 * so far and in front of those issued after it; it settles a pending frr_clear first (never fused), reads the current target
 * set (own or caller-bound, one or two frames in flight), writes no target, touches no field of frr_stats, leaves the latest
 * geometry pass as it is and waits for nothing on the host.  It is logged and replayed: behind a failed command it writes
 * nothing and runs again with it, under the uniforms of the call.  A later frr_draw_list_if of this ctx that names the buffer
 * is already ordered behind it; the caller orders its own reads with frr_frame_fence or frr_sync.
 * On a partitioned ctx the region, the rectangle's pixels and the window's pixels are those of the tile rows this rank owns
 * (an item with none: OUTSIDE): the answer is the rank's own, "would this item change a pixel of mine", which is what the
 * rank's frr_draw_list_if needs.  The ranks' values do NOT add up to the unpartitioned ones.
 * frr_query_boxes_host: the same through a temporary device buffer into host memory; a synchronisation point; *nunits
 * (optional) receives n.
 * Errors: the list errors of frr_draw_list (FRR_ERR_INVALID: unknown, freed or dead); FRR_ERR_INVALID for a list without a
 * bounds table (frr_last_error names frr_drawlist_bounds); the window and buffer errors of frr_visible_pixels.  A refused call
 * leaves the ctx drawing.  out_entries == 0 (after these checks): FRR_OK, nothing happens.
 * The pyramid is a buffer of the ctx, allocated for the whole viewport on first use and never grown: no command waits for it.
 * frr_profile_get("k_boxes"): the launches of both calls.  Option "box_bounds_chunks" (0 .. 1024; 0: the default, 1,024) caps
 * the workgroups frr_drawlist_bounds gives one mesh -- a test hook for its stride loop; the table does not depend on it. */
int frr_drawlist_bounds(frr_ctx *ctx, int list, float *host_lo_hi, uint32_t *host_flags, uint64_t cap, uint64_t *nitems);
int frr_query_boxes(frr_ctx *ctx, int list, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                    void *dev_out_u32, uint64_t out_entries);
int frr_query_boxes_host(frr_ctx *ctx, int list, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                         uint32_t *host_out, uint64_t out_entries, uint64_t *nunits);
/* host build of the whole rule over arrays (no ctx, no device): mvps [nitems][16], lo_hi [nitems][6], flags [nitems]; depth
 * addressed as above (depth_entries: how many it holds); row_owned: NULL, or one byte per window-local tile row (32 pixel
 * rows), non-zero where the rank owns it.  The region's minimum is a plain walk over its pixels.  status_rect_level (or NULL):
 * [nitems][6] = status (0 NONE, 1 OUTSIDE, 2 HIDDEN, 3 KEPT, 4 UNBOUNDED), the clamped rectangle rx0, ry0, rx1, ry1
 * (window-local, inclusive) and the level.  Returns nitems, or -1 for arguments frr_query_boxes would refuse. */
int64_t frr_host_query_boxes(const float *mvps, const float *lo_hi, const uint32_t *flags, uint64_t nitems,
                             uint32_t W, uint32_t H, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                             const float *depth, uint64_t depth_entries, const uint8_t *row_owned,
                             uint32_t *out, uint64_t out_entries, int32_t *status_rect_level);

/* Stream-side fence, no host wait: `stream` (a hipStream_t of the caller; NULL = the ctx's stream) waits for every frame
 * issued so far, so that what the caller enqueues on it next sees their targets.  Needed with option bound_targets_in_flight
 * (below) and by callers that read the ctx's own targets (frr_target_ptrs) on a stream other than the ctx's; also the way to
 * order an in-place rewrite of a device-bound mesh behind the draws that still read it (frr_create).
 * The frames it fences are whole: like the reference's draw (renderer.rs:269-384 has no failure path) a draw of this
 * library cannot fail -- a raster pass whose need of the internal work lists is not known to fit is checked on the host,
 * and repaired, before frr_raster / frr_draw returns (the call then waits for the pass's binning launch, not for its tile
 * kernel; a pass that repeats a mesh registration, uniforms -- texture pointers and sizes included --, window and partition
 * already seen to fit, with no frr_texture_upload since and, for a device-bound mesh, no frr_sync since, is not waited
 * for).  What is not whole at a fence: commands issued behind a frr_geometry* that no frr_raster has followed yet (an open
 * or abandoned pass).  Nothing has verified that pass, so if it found the fan space too small they have written nothing, and
 * they are replayed at the next synchronisation point only (frr_resolve_varyings says so for itself; the same holds for
 * frr_draw_lines, frr_draw_wireframe, frr_shade_varyings, frr_shade_items and frr_visible_pixels there).  A caller that
 * fences such a frame calls frr_sync first.
 * `stream` has to stay alive until the second frr_clear from now when it fenced the ctx's OWN targets (that frr_clear
 * records an event on it: frr_target_ptrs). */
int frr_frame_fence(frr_ctx *ctx, void *stream);
/* The reverse edge: the next kernel that WRITES the frame targets (the pending frr_clear, the next tile kernel) waits for
 * what `stream` (NULL = the ctx's stream) holds now -- e.g. an exchange that still reads a caller-bound target set which is
 * about to be bound for a new frame under option bound_targets_in_flight, where no frame work runs on the ctx's stream.
 * Calls add up: after frr_frame_wait on several streams that write waits for all of them.  "That write" is the first one
 * issued after the call (a frr_clear or frr_raster / frr_draw from then on); a write issued before it that the library
 * performs later -- a deferred clear of the targets bound before, run by frr_bind_targets -- waits too, but does not
 * take the wait away from it.
 * (The ctx's OWN targets need no such call: the library orders a set's next frame behind whatever was queued on the stream
 * the set's pointers were handed to by frr_target_ptrs / frr_frame_fence, up to the frr_clear that starts that frame.) */
int frr_frame_wait(frr_ctx *ctx, void *stream);
/* Synchronisation point: waits for everything issued so far (both streams).  Caller-bound targets are defined, and a
 * draw that needed a larger work list has been replayed (FRR_ERR_CAPACITY), when this -- or frr_readback,
 * frr_get_stats, frr_readback_setup, frr_geometry with a count -- returns. */
int frr_sync(frr_ctx *ctx);
/* FrameBuffer::get_data (renderer.rs:473-475) + depth + triangle ids -> host; NULLs skipped.
 * tri_id holds, per depth-buffer index, the global emission index (over the draws since the last
 * frr_clear) of the triangle owning the pixel, 0xFFFFFFFF where nothing was drawn. */
int frr_readback(frr_ctx *ctx, uint8_t *rgba, float *depth, uint32_t *tri_id);
/* Vec<[Vertex;3]> of the last frr_geometry, [n][3] frr_setup_vertex, emission order */
int frr_readback_setup(frr_ctx *ctx, frr_setup_vertex *out, uint64_t cap_tris, uint64_t *ntris);
int frr_get_stats(frr_ctx *ctx, frr_stats *out);

/* ---- timing on the ctx stream (HIP events) -------------------------------------------------- */
/* slot in [0,16): record an event now; elapsed in ms between two recorded slots (syncs on `b`). */
int frr_event_record(frr_ctx *ctx, int slot);
int frr_event_elapsed_ms(frr_ctx *ctx, int a, int b, float *ms);
/* Development and test switches of a ctx (frr_set_option(ctx, name, value); unknown name or bad value: FRR_ERR_INVALID).
 * None changes a result: every path is held to the same oracle by the tests.  The library itself reads no environment
 * variable; the Python binding maps FRR_* variables onto these for the test-suite and the tools.
 *   "raster_sweep"            1: brute-force tile kernel (one triangle per wavefront) instead of the span kernel
 *   "raster_nw", "raster_occ" waves per tile workgroup (3, 4, 6, 8, 16) / waves per SIMD its registers are budgeted for
 *                             (4, 6, 8); 0 = chosen per launch
 *   "bin_chunks"              number of chunk workgroups of the segmented binning (0 = by mesh size)
 *   "bin_atomics"             1: global-atomic CSR binning (the path for windows of more than 36,864 tiles)
 *   "bin_capacity"            initial capacity of the (triangle, tile) lists in records (tests of the replay)
 *   "fan_capacity"            initial capacity of the fan space in triangles (the same)
 *   "frames_in_flight"        2 (default): with the ctx's OWN targets a frame that starts with frr_clear takes the other of two target
 *                             sets and the other of two streams, so that two frames are in flight (frr_readback / frr_target_ptrs join
 *                             them; frr_target_ptrs returns the current frame's pointers); 1: one target set, one stream
 *   "bound_targets_in_flight" 1: the same for caller-bound targets -- every frame runs on one of two PRIVATE streams (none of it on
 *                             the ctx's stream); the caller binds a different target set for each of two consecutive frames and orders
 *                             its reads with frr_frame_fence (bench.py's multi-GPU loop).  Default 0: everything that touches
 *                             caller-bound targets runs on the ctx's stream, in call order
 *   "overlap"                 frames that are NOT in flight as above: 2 (default) geometry + binning of a pass WITH VARYINGS run on a
 *                             further private stream beside the previous pass's tile kernel (measured to pay there only); 1: of every
 *                             pass; 0: one stream, one kernel after the other
 *   "tile_slot_records"       records per tile slot of the near-first copy (tests of its overflow arena)
 *   "clip_queue"              1: clipped inputs beyond four per 256-triangle block are expanded by a second launch
 *                             (k_geom_clip, one wavefront each over the whole chip) instead of by their block; 0: never;
 *                             -1 (default): when the counters last read back (frr_sync, frr_readback, frr_get_stats)
 *                             showed a block with more than 16 clipped inputs
 *   "clear_eager"             1: frr_clear runs its own kernel at once instead of riding on the next full-window draw
 *   "lines_chunk"             a test hook like bin_capacity: iterations one segment contributes to a round of its wavefront in the
 *                             line kernels (0 = default 2^24, the bound that keeps a wavefront's prefix sums in 32 bits).  Only a
 *                             segment nearly as long as a 2^24-pixel buffer takes a second round at the default; a small value
 *                             lets the tests walk that path on a 96 x 70 frame
 *   "visible_lds_bins"        a test hook like lines_chunk: v > 0: a frr_visible_pixels whose histogram can meet more than v units (the
 *                             pass's items, or out_entries if that is fewer; per triangle: out_entries) adds to global memory
 *                             directly instead of through the LDS histogram; 0 = default, the 4,096 units the LDS path takes.
 *                             The small test frames can then walk both paths
 *   "tile_order"              which workgroup of the tile kernel takes which tile (segmented binning): 0 (default) the fixed order
 *                             by position; 1 heaviest first -- each XCD's run of neighbouring tiles by descending records in the
 *                             latest pass over the same grid on the same workspace (the fixed order on a first pass, after a new
 *                             window / partition / workgroup shape, on replays, and always above 4,096 tiles; measured no faster
 *                             than 0); 2 a seeded random permutation (tests) */
int frr_set_option(frr_ctx *ctx, const char *name, int64_t value);
/* per-kernel accumulated device time (ms) and launch count since frr_profile_reset.  `mask`:
 * 0 = off, -1 = every kernel, else OR of (1 << index) with index in the order k_clear,
 * k_geom, k_geom_scan, k_bin_count, k_tile_scan, k_bin_fill, k_raster,
 * k_bin_seg, k_lines_mark, k_lines_paint, k_visible (k_visible covers the launch that zeroes the counts and builds the item
 * boundaries too; k_geom covers the clip kernel too when the clip queue is in use, and the kernel that fills an instanced pass's matrices).  A profiled launch is bracketed by two
 * HIP events on the ctx stream. */
int frr_profile_enable(frr_ctx *ctx, int mask);
/* bracket only every `period`-th launch of each selected kernel (default 1): an event pair costs the
 * stream ~4 us, which matters when the whole frame is 150 us; frr_profile_get then reports the sampled
 * launches. */
int frr_profile_set_period(frr_ctx *ctx, uint32_t period);
/* raster passes since frr_create whose tile kernel took a built block -> tile order (option "tile_order" 1 or 2; tests) */
int frr_tile_order_passes(frr_ctx *ctx, uint64_t *passes);
int frr_profile_reset(frr_ctx *ctx);
int frr_profile_get(frr_ctx *ctx, const char *kernel, float *total_ms, uint32_t *launches);

/* ---- host helpers mirroring matrix_util.rs:3-35 (pure host arithmetic, no device) --------- */
void frr_set_identity(float m[16]);
void frr_set_look_at(const float eye[3], const float at[3], const float up[3], float m[16]);
void frr_set_perspective(float fovy, float aspect, float zn, float zf, float m[16]);

/* ---- debug / parity hooks ----------------------------------------------------------------- */
/* device evaluation of the library's atan2f (bit-exact fdlibm port) on n (y,x) pairs */
int frr_debug_atan2f(frr_ctx *ctx, const float *y, const float *x, float *out, uint64_t n);
/* the same source compiled for the host, to pin the port against glibc without a GPU */
float frr_host_atan2f(float y, float x);
/* the line kernels' per-iteration arithmetic compiled for the host (cf. frr_host_atan2f): the linear pixel indices
 * y * width + x that draw_line(x1, y1, x2, y2) paints, in write order; returns their number (written up to cap) */
int64_t frr_host_line_pixels(uint32_t x1, uint32_t y1, uint32_t x2, uint32_t y2, uint32_t width, uint64_t *out, uint64_t cap);
/* host build of the device's per-instance matrix product (cf. frr_host_atan2f, frr_host_line_pixels):
 * out = (proj * view) * model, column-major, every element ((a0*b0 + a1*b1) + a2*b2) + a3*b3 */
void frr_host_instance_mvp(const float proj[16], const float view[16], const float model[16], float out[16]);
/* host build of the device's item search of a list pass (cf. frr_host_line_pixels): the item i with
 * first[i] <= t < first[i] + ntris[i], or -1; first is the exclusive prefix of ntris (it repeats where items are empty) */
int64_t frr_host_list_item(const uint32_t *first, const uint32_t *ntris, uint64_t nitems, uint32_t t);
/* host build of the span logic of frr_visible_pixels (cf. frr_host_list_item): the unit search, the run heads and the run
 * lengths, span by span and lane by lane as the kernel takes them, over an id array of id_entries u32 and a window
 * (x0 >= 0; the window's last index (y1 - y0 - 1) * x1 + (x1 - x0) - 1 lies inside the array).  bounds: the nunits + 1
 * non-decreasing boundaries of the items (the ids of item k are [bounds[k], bounds[k + 1])), or NULL: per triangle, the units
 * are the ids 0 .. nunits.  Every one of the out_entries entries of out is written, as by frr_visible_pixels.  Returns the
 * number of adds -- run heads that counted for a unit --, or -1 for a bad argument. */
int64_t frr_host_visible_counts(const uint32_t *ids, uint64_t id_entries, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                                const uint32_t *bounds, uint64_t nunits, uint32_t *out, uint64_t out_entries);
/* host build of the per-entry item lookup of frr_shade_items (cf. frr_host_visible_counts): over the same kind of id array,
 * window and nitems + 1 boundaries (never NULL), span by span and lane by lane as the kernel takes them -- the span's
 * smallest and largest in-pass id, the narrowed range, each lane's search.  item_out has id_entries entries, addressed like
 * ids: every entry of the window receives its item, or 0xFFFFFFFF where the id is not one of the pass's; entries outside
 * the window are not written.  Returns the number of (span, distinct item) rounds -- a span shades once per distinct
 * item its lanes hold --, or -1 for a bad argument.  nitems == 0: every entry of the window is 0xFFFFFFFF, 0 rounds. */
int64_t frr_host_entry_items(const uint32_t *ids, uint64_t id_entries, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                             const uint32_t *bounds, uint64_t nitems, uint32_t *item_out);
/* host build of the device's facing determinant (frr_set_cull; cf. frr_host_atan2f): d of the three clip positions
 * clip[0..3], clip[4..7], clip[8..11] (x, y, z, w each) */
float frr_host_cull_det(const float clip[12]);
/* MVP x vertex contraction of a pos3/uv2/normal3 mesh with the current uniforms: clip xyzw per vertex
 * (ntris*3*4 floats) by the exact VALU form (use_mfma = 0, glam's association) or by
 * v_mfma_f32_16x16x4_f32 (use_mfma = 1, an fmaf chain: NOT bit-identical); *ms = kernel time. */
int frr_debug_mvp(frr_ctx *ctx, int mesh, int use_mfma, float *clip_out, float *ms);
/* PMC calibration: gathers 2^log2_records distinct 64-byte records (true bytes = 64 << log2_records) */
int frr_debug_gather_calib(frr_ctx *ctx, uint32_t log2_records);
/* device wave64 inclusive prefix sum (DPP) of 64 values, for tests */
int frr_debug_scan64(frr_ctx *ctx, const uint32_t *in, uint32_t *out);
/* the three-instruction reciprocal of the fragment loop (frr_exact.h: recip_exact) against the IEEE
 * division, and the shaders' 1/sqrt (rsqrt_exact) against 1.0f / sqrtf, for every f32 bit pattern in
 * [lo_bits, hi_bits): number of differing results and the smallest offending pattern (0xFFFFFFFF if none). */
int frr_debug_rcp_check(frr_ctx *ctx, uint32_t lo_bits, uint32_t hi_bits, uint64_t *mismatches, uint32_t *first_bad);

#ifdef __cplusplus
}
#endif
#endif
