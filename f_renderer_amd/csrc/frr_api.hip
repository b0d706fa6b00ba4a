// frr_api.hip -- host side of libfrr_hip.so: the C ABI of include/frr.h over the kernels in
// frr_kernels.h.  gfx950 only; no CPU fallback (every compute entry point needs the device).
#include "frr_kernels.h"
#include "frr_tile_order.h"
#include "frr_rules.h"
#include "frr_proof.h"
#include "frr_lines.h"
#include "frr_varyings.h"
#include "frr_shade.h"
#include "frr_visible.h"
#include "frr_query.h"
#include "frr_boxes.h"
#include "frr_own.h"

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <hip/hiprtc.h>

#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

// The text of the device headers, for frr_shader_register (hiprtc compiles user shaders into the library's own kernels):
// the assembler copies the files into .rodata of the host object.
#ifndef FRR_CSRC_DIR
#define FRR_CSRC_DIR "f_renderer_amd/csrc"   // (builds started at the repository root; f_renderer_amd/_native.py passes the absolute path)
#endif
#if !defined(__HIP_DEVICE_COMPILE__)
#define FRR_EMBED(sym, file) __asm__(".pushsection .rodata\n.global " #sym "\n" #sym ":\n.incbin \"" FRR_CSRC_DIR "/" file "\"\n.byte 0\n.popsection\n")
FRR_EMBED(frr_src_device_h, "frr_device.h");
FRR_EMBED(frr_src_exact_h, "frr_exact.h");
FRR_EMBED(frr_src_kernels_h, "frr_kernels.h");
FRR_EMBED(frr_src_raster_h, "frr_raster.h");
FRR_EMBED(frr_src_shade_h, "frr_shade.h");
FRR_EMBED(frr_src_visible_h, "frr_visible.h");
FRR_EMBED(frr_src_frr_h, "../../include/frr.h");
#endif
extern "C" const char frr_src_device_h[], frr_src_exact_h[], frr_src_kernels_h[], frr_src_raster_h[], frr_src_shade_h[], frr_src_visible_h[], frr_src_frr_h[];

using namespace frr;
static_assert(PASS_FAN_BITS == FAN_BITS && MAX_PASS_INPUTS << FAN_BITS == 1ull << PASS_ORDER_KEY_BITS, "frr_rules.h: an input's order keys are 32 * input + (0 .. 31), in 32 bits (frr_device.h)");

namespace {

enum KernelId { KID_CLEAR, KID_GEOM, KID_GEOM_SCAN, KID_BIN_COUNT,
                KID_TILE_SCAN, KID_BIN_FILL, KID_RASTER, KID_BIN_SEG, KID_LINES_MARK, KID_LINES_PAINT, KID_VISIBLE, KID_BOXES, KID_COUNT };
const char *const kKernelNames[KID_COUNT] = {"k_clear", "k_geom", "k_geom_scan",
                                             "k_bin_count", "k_tile_scan", "k_bin_fill",
                                             "k_raster", "k_bin_seg", "k_lines_mark", "k_lines_paint", "k_visible", "k_boxes"};

struct Mesh {
    DevBuf<float> own_dev; DevBuf<uint32_t> own_idx;   // a host upload: the library's copies (dev / idx point at them); else empty, and dev AND idx are the caller's
    const float *dev = nullptr;    // [ntris][3][NF], or with idx: the vertex array [nverts][NF]
    const uint32_t *idx = nullptr; // indexed mesh (frr_mesh_upload_indexed): [ntris][3] vertex numbers, all < nverts when registered
    uint64_t nverts = 0, ntris = 0;
    bool used = false;
    int vs = 0;
    uint64_t gen = 0;   // which registration of the ctx this is (DrawSig: a later mesh may live at a freed one's address)
};
struct Texture {
    DevBuf<uint8_t> dev;
    uint32_t w = 0, h = 0;
};
// a list of draw_line calls (frr_lines_upload / frr_lines_bind_device): every segment's walk stays inside the buffer
struct Lines {
    DevBuf<uint4> own_xyxy; DevBuf<uint32_t> own_rgba;   // a host upload: the library's copies; else empty
    const uint4 *xyxy = nullptr;     // [n] {x1, y1, x2, y2}
    const uint32_t *rgba = nullptr;  // [n]
    uint64_t n = 0;
    bool used = false;
};
// an instance table (frr_instances_upload / frr_instances_bind_device): one model matrix per instance of an instanced pass
struct Instances {
    DevBuf<float> own;             // a host upload: the library's copy; else empty, and dev is the caller's
    const float *dev = nullptr;    // [n][16], column-major like frr_uniforms.model
    uint64_t n = 0;
    bool used = false;
    uint64_t gen = 0;              // which registration of the ctx this is (DrawSig, like Mesh::gen)
};
// a material table (frr_materials_upload / frr_materials_bind_device): one frr_material per item of a pass (frr_shade_items)
struct Materials {
    DevBuf<frr_material> own;          // a host upload: the library's copy; else empty, and dev is the caller's
    const frr_material *dev = nullptr; // [n], 16-byte aligned, every entry material_ok when registered
    uint64_t n = 0;
    uint32_t slots = 0;                // bit s: some entry names texture slot s (a lit shader needs a texture there)
    bool used = false;
};
// a draw list (frr_drawlist_upload): a snapshot of its items -- per item the mesh's pointers, counts and generation, and the
// model matrix -- so a pass over it reads nothing of frr_ctx::meshes.  Freeing a mesh it names kills it for good (dead).
struct DrawList {
    DevBuf<ListRow> rows;          // [n] GeomArgs::items
    DevBuf<uint32_t> first;        // [2 n] first[n] | ntris[n]: GeomArgs::item_first / item_ntris
    DevBuf<float> models;          // [n][16] the k_instance_mvp input
    std::vector<ListRow> hrows;    // [n] the host's copy of `rows` (frr_drawlist_bounds: the distinct meshes of the snapshot)
    // frr_drawlist_bounds: per item the object-space box of its mesh and the flags (frr_boxes.h); frr_query_boxes reads them
    DevBuf<float> box_lo_hi; DevBuf<uint32_t> box_flags; bool has_bounds = false;
    std::vector<int> mesh; std::vector<uint64_t> mesh_gen;   // [n] who the rows were taken from (frr_mesh_free)
    uint64_t n = 0, total = 0;     // items, and the sum of their triangle counts (< 2^27)
    int vs = FRR_VS_CLIP;          // the one vertex shader of all items (no items: any pixel shader goes with nothing)
    bool any_dev = false;          // some item's mesh is device-bound (DrawSig: sync_epoch)
    bool dead = false;
    bool used = false;
    uint64_t gen = 0;              // which upload of the ctx this is (DrawSig, Cmd: an id is reused)
};
// slot tables (frr_ctx::meshes, lines, instances, lists): a record goes into the first unused slot, or behind the last; its index is its id
template <typename R> int slot_put(std::vector<R> &v, R &&r)
{
    size_t i = 0;
    while (i < v.size() && v[i].used) ++i;
    if (i < v.size()) v[i] = std::move(r); else v.push_back(std::move(r));
    return (int)i;
}
template <typename R> bool slot_ok(const std::vector<R> &v, int id) { return id >= 0 && id < (int)v.size() && v[(size_t)id].used; }
struct ProfRec { int kid; Event a, b; };

// ---- user shaders (frr_shader_register): a per-process registry of code objects, loaded per ctx on first use ---------
constexpr int kSpanShapes[6][2] = {{16, 4}, {8, 6}, {6, 6}, {4, 8}, {4, 6}, {LIGHT_NW, 6}};   // the shapes launch_raster knows
struct UserShader {
    int nf = 0, K = 0;
    std::vector<char> code;
    std::string geom_inst[2], clip_inst[2];   // ... of an instanced pass ([indexed mesh])
    std::string geom_list, clip_list;         // ... of a list pass
    std::string geom, clip, geom_idx, clip_idx, sweep, entries, span[2][6], shade[2], shade_items[2];   // lowered kernel names (geom_idx / clip_idx: the geometry kernels of an indexed mesh; [count fragments][shape]; sweep: the brute-force tile kernel; shade / shade_items: k_shade_vary / k_shade_items [16-byte loads])
};
std::mutex g_shader_mu;
std::vector<UserShader *> g_shaders;      // id = FRR_SHADER_USER_BASE + index; never shrinks
const UserShader *user_shader(int id)
{
    std::lock_guard<std::mutex> lk(g_shader_mu);
    const int i = id - FRR_SHADER_USER_BASE;
    return (i >= 0 && i < (int)g_shaders.size()) ? g_shaders[(size_t)i] : nullptr;
}
// The library's private streams are recycled across contexts (per device): a process's HIP streams are mapped onto a handful
// of hardware queues in creation order, and a ctx created after others must not end up with its two frame streams -- or a frame
// stream and the caller's -- on one queue (two streams that share a queue run nothing beside each other).  Recycling keeps the
// queues a process's contexts use the same few from the first context to the last.
std::mutex g_stream_mu;
std::map<int, std::vector<hipStream_t>> g_stream_pool;
hipError_t acquire_stream(int device, hipStream_t *out)
{
    {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        std::vector<hipStream_t> &v = g_stream_pool[device];
        if (!v.empty()) { *out = v.back(); v.pop_back(); return hipSuccess; }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
void release_stream(int device, hipStream_t st)
{
    if (!st) return;
    (void)hipStreamSynchronize(st);
    std::lock_guard<std::mutex> lk(g_stream_mu);
    g_stream_pool[device].push_back(st);
}

struct UserModule {
    hipModule_t mod = nullptr;
    hipFunction_t geom_inst[2] = {}, clip_inst[2] = {}, geom_list = nullptr, clip_list = nullptr;
    hipFunction_t geom = nullptr, clip = nullptr, geom_idx = nullptr, clip_idx = nullptr, sweep = nullptr, entries = nullptr, span[2][6] = {}, shade[2] = {}, shade_items[2] = {};
};

// One of the ctx's private frame streams (frr_ctx::tstream) and what orders it against the other streams.
struct FrameStream {
    hipStream_t st = nullptr;
    Event ev;                  // joins it into a caller's stream (fence_stream)
    bool dirty = false;        // it holds work `stream` has not waited for
    bool xdirty = false;       // ... that the stream of the latest frr_frame_fence (frr_ctx::xfence) has not waited for
    uint32_t joined = 0;       // the join_epoch in which it last waited for `stream` (gstream_join)
};
// The tile kernel that last read a workspace set: the second stream waits for it before it overwrites the set.
struct ReaderFence {
    Event ev; bool pending = false;                // fires when the latest tile kernel that reads this set is done
    hipStream_t stream = nullptr;                  // ... on this stream
    bool recorded = false;                         // the event was recorded right behind that kernel
};

// Workspace of one geometry pass / one raster pass.  There are two of each, used alternately (parity of the pass), so
// that the geometry + binning kernels of pass n + 1 can run on the ctx's second stream while the tile kernel of pass n
// still reads what pass n left (frr_device.h: GeomTab / BinTab are the device-side halves of the same scheme).
struct GeomSet {
    DevBuf<uint32_t> block_sums;     // per 256-triangle block: triangles emitted
    DevBuf<uint32_t> block_prefix;   // ... and their exclusive scan
    DevBuf<uint32_t> tinfo;          // per input: fan size | emission offset in its block
    DevBuf<uint32_t> fanbase;        // per clipped input: first fan slot
    DevBuf<uint32_t> fan_okey;       // per fan slot: order key within the draw
    DevBuf<RasterRec> recs;          // [input triangles + fan capacity]: the setup capacity, recs.cap()
    DevBuf<float> vary;              // floats
    DevBuf<uint4> pbox;              // [recs.cap()]
    DevBuf<uint32_t> bcount;         // [geometry blocks] dense binning entries per block (GeomArgs::bcount)
    DevBuf<uint2> clipq;             // [input triangles] the clip kernel's queue (GeomArgs::clipq)
    DevBuf<float> inst_tab;          // [instances][32] the matrices of an instanced pass (GeomArgs::inst)
    DevBuf<uint32_t> keep_tab;       // [items] the keep table of a predicated list pass (GeomArgs::keep), beside its matrices
    // frr_resolve_varyings: emission index within the draw -> slot, one table per parity of the geometry pass (allocated by
    // the first resolve of a pass on this set, at the set's setup capacity); vslot_stream: the stream of its latest user
    DevBuf<uint32_t> vslot[2]; hipStream_t vslot_stream[2] = {nullptr, nullptr};
    // the geometry pass (its sequence number, in which epoch) whose table the latest resolve built: a later resolve of the same
    // pass skips k_vary_slots.  A replay starts a new epoch, so a table a cancelled launch never built is built by the replay.
    uint32_t vslot_seq[2] = {0, 0}, vslot_epoch[2] = {0, 0};
    ReaderFence reader;
};
struct BinSet {
    DevBuf<uint4> bins;            // 16-byte cull records, one per (triangle, tile) pair
    DevBuf<uint4> bins2;           // the same in near-first order per tile (tile kernel pre-pass)
    DevBuf<uint32_t> bin_matrix;   // [G][ntiles] per-chunk tile histograms
    DevBuf<uint32_t> tile_cost;    // [ntiles] records per tile of the latest tile kernel on this set
    DevBuf<uint32_t> tile_perm;    // [ntiles] block -> tile order of the current pass (option tile_order)
    bool cost_known = false; TileOrderKey cost_key = {};       // tile_cost was written by a pass with this key (frr_tile_order.h)
    ReaderFence reader;
};

// Everything a command reads and changes on the host.  Every logged command carries the state it started from, so that
// the commands from a failed one onwards can be replayed (finish()).  Its parts:

// Bound: set by the calls between commands, so a replay gives every command its own copy and puts the current one back afterwards.
struct Bound {
    uint8_t *color = nullptr; float *depth = nullptr; uint32_t *tri_id = nullptr; // the frame targets (own or caller-bound)
    int tset = 0;                                                                 // which of the ctx's own target sets is current
    int rank = 0, world = 1; bool part_blocked = false;                           // tile-row ownership (frr_set_partition*)
};
// frr_clear is deferred: the first full-window draw of the span kernel performs it inside the tile kernel
// (keys start from the clear depth, every pixel of the tile is written); anything else that looks at the
// targets first settles it with k_clear.  option clear_eager restores the immediate clear.
struct Clear {
    bool pending = false;          // targets not cleared yet
    bool unowned_debt = false;     // partitioned ctx: the tile rows of other ranks missed a fused clear
    int debt_tiles_y = 0;          //   (tile rows of the window of the draw that left the debt)
    uint32_t rgba = 0; float depth = 0.0f;
    uint32_t wait_serial = 0;      // frr_frame_wait calls before the pending frr_clear was issued (frr_ctx::waits)
};
// The latest geometry pass: what it read (frr_proof.h: the half a raster pass's signature takes), and what it left for the commands behind it.
struct GeomPass {
    GeomRead read;
    int part_rank = 0, part_world = 1; bool part_blocked = false;   // the partition read.filter was built under (raster_check)
    uint32_t fan_cap = 0;          // fan capacity it was launched with
    uint32_t nblocks = 0;
    uint32_t seq = 0;              // its sequence number
    bool scan_pending = false;     // its block sums are not scanned yet (geom_scan: by the binning launch, or k_geom_scan)
    int set = 0;                   // its workspace set (GeomSet)
    bool on_g = false;             // it runs on the second stream (its binning follows it there)
    // its items (frr_geometry_item_ranges): the items of a list pass, the instances of an instanced pass (stride inputs each), else one
    uint64_t nitems = 1, stride = 0;
    bool pred = false;             // it is a predicated list pass: what it needs of the work lists hangs on device data (never proven)
    bool none() const { return read.vs < 0; }      // no geometry pass yet
    void setup_list_gone() { read.ntris = 0; }     // frr_clear: frr_raster then draws nothing (nitems stays: frr_visible_pixels_host reports it)
};
struct FrameState {
    Bound bound;
    Clear clear;
    uint32_t frame_no = 1;         // frr_clear count (device statistics are tagged with it)
    uint64_t tris_in = 0; uint32_t draws = 0;   // statistics the host knows: inputs submitted / geometry passes since frr_clear
    int lane = 0;                  // which of the two sets of device tables this frame's passes use (frr_device.h: Lane)
    int gpars[2] = {0, 0}, bpars[2] = {0, 0};   // per lane: parity of the latest geometry / raster pass (GeomTab / BinTab)
    int gpar() const { return gpars[lane]; }
    int bpar() const { return bpars[lane]; }
    int bset = 0;                  // workspace set of the latest raster pass (BinSet)
    GeomPass geom;
};

struct Cmd {
    enum Kind { GEOM, RASTER, LINES, VARY, SHADE, VISIBLE, SHADE_ITEMS, BOXES } kind;
    // GEOM and RASTER own device tables (GeomTab / BinTab), which finish() resets before it replays them.  The other six own
    // none and are replayed by running them again; what tells them apart is two traits -- does the command read the latest
    // pass's tables (VARY, VISIBLE, SHADE_ITEMS, a wireframe LINES), and does it write a target (LINES, SHADE, SHADE_ITEMS);
    // BOXES does neither: cmd_settle / cmd_stream / cmd_done
    bool owns_table() const { return kind == GEOM || kind == RASTER; }
    FrameState pre;            // host state before the command
    uint32_t seq = 0;          // sequence number of its latest execution
    DevUniforms duni;          // uniforms at the time of the call
    // GEOM
    int mesh = -1; bool filter = false; int32_t fy0 = 0, fy1 = 0;
    int cull = FRR_CULL_NONE;           // frr_set_cull at the time of the call (a replay runs the pass under it again)
    int list = -1; uint64_t list_gen = 0;   // a list pass: its list, and which upload that id meant (mesh is unused then; pv as below)
    // a predicated list pass (frr_geometry_list_if): the caller's device buffer, read again by a replay, and the threshold
    bool pred = false; const uint32_t *keep = nullptr; uint64_t keep_entries = 0; uint32_t min_value = 0;
    int inst = -1; float pv[16] = {};   // an instanced pass: its table, and proj * view at the time of the call (the table's mvp = pv * model)
    // RASTER
    int ps = 0; int32_t x0 = 0, x1 = 0, y0 = 0, y1 = 0; bool count_frags = true;
    // LINES: a list, or (lines < 0) the wireframe of the latest geometry pass in one colour
    int lines = -1; uint32_t wire_rgba = 0;
    // VARY (frr_resolve_varyings): the window in x0 .. y1 and the caller's buffer
    float *vary_out = nullptr;
    // SHADE (frr_shade_varyings): the window in x0 .. y1, the shader in ps, the buffer ([shade_entries][shade_K]: the caller's,
    // or one of frr_ctx::shade_tmp) and the range of triangle ids
    const float *shade_in = nullptr; uint64_t shade_entries = 0; int shade_K = 0; uint32_t id_first = 0, id_count = 0;
    // SHADE_ITEMS (frr_shade_items): SHADE's window, shader and buffer (no id range), and the material table -- a view: the
    // table cannot go while the command is logged (frr_materials_free finishes first), and a replay reads it again
    const frr_material *mats = nullptr;
    // VISIBLE (frr_visible_pixels): the window in x0 .. y1, the unit and the caller's buffer
    int vis_unit = 0; uint32_t *vis_out = nullptr; uint64_t vis_entries = 0;
    // frr_query_pixels: a RASTER command that counts instead of drawing (exec_raster), with VISIBLE's unit and buffer -- or, where
    // there is nothing to rasterize, a VISIBLE command that only zeroes the buffer
    bool query = false;
    // BOXES (frr_query_boxes): the window in x0 .. y1, the list in list / list_gen, proj * view of the call in pv, VISIBLE's buffer
    int par = 0;               // the parity it ran with (finish(): which table a failed command left behind; LINES: of the geometry pass a wireframe read)
    int set = 0;               // RASTER: the BinSet it ran with
    int lane = 0;              // the lane of device tables it ran in
};

static_assert(std::is_trivially_copyable<FrameState>::value && std::is_trivially_copyable<Cmd>::value, "the replay copies them: views only, no owner");
inline uint64_t fnv1a(const void *p, size_t n, uint64_t h = 1469598103934665603ull)
{
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
    return h;
}
// GeomRead::duni_hash: every field a vertex shader can read (field ranges without padding: the struct has some in front of its texture pointer)
inline uint64_t geom_uniform_digest(const DevUniforms &du)
{
    uint64_t h = fnv1a(&du, offsetof(DevUniforms, flat_color) + sizeof du.flat_color);
    h = fnv1a(&du.tex, offsetof(DevUniforms, tex_h) + sizeof du.tex_h - offsetof(DevUniforms, tex), h);
    h = fnv1a(du.user, sizeof du.user, h);
    return fnv1a(du.slot_tex, offsetof(DevUniforms, slot_h) + sizeof du.slot_h - offsetof(DevUniforms, slot_tex), h);
}

} // namespace

struct frr_ctx {
    int device = 0;
    uint32_t W = 0, H = 0;
    hipStream_t stream = nullptr;   // the caller's stream (or a private one): tile kernels, clears, copies -- everything that touches the targets
    hipStream_t gstream = nullptr;  // private: geometry + binning of the next pass, beside the tile kernel of the current one
    bool own_stream = false;
    int overlap = 2;                // option overlap: 0 never use gstream, 1 always, 2 (default) for passes with varyings (exec_geometry)
    bool g_used = false;            // some pass has run on gstream since the streams were last drained (cross-stream events are needed)
    // The ctx's own frame targets: TWO sets.  A frame that starts with frr_clear on own targets takes the other set and
    // its tile kernels the other tile stream (tstream[1] for set 1), so that the tile kernel of frame n + 1 fills the drain
    // of frame n's (2,040 tiles on 1,536 workgroup slots end with a third of the chip idle).  Nobody can look at own targets
    // except through this library (frr_readback, frr_target_ptrs, which join the streams first), so the only visible
    // change is that frr_target_ptrs' pointers are those of the CURRENT frame.  Caller-bound targets: one set, one stream.
    DevBuf<uint8_t> own_color[2]; DevBuf<float> own_depth[2]; DevBuf<uint32_t> own_tri_id[2];
    // The private frame streams, by target set index (tstream_of).  [1]: everything of the frames that use own target set 1
    // (or, option bound_targets_in_flight, of every other frame); [0], option bound_targets_in_flight: the frames in between
    // (the caller's stream then carries no frame work at all).  [1] is acquired first (frr_clear), and calls that go over
    // both go over [1] first.
    FrameStream tstream[2];
    hipStream_t xfence = nullptr;    // the stream of the latest frr_frame_fence (FrameStream::xdirty)
    bool bound_in_flight = false;    // option bound_targets_in_flight: frames on caller-bound targets alternate between the two private streams too;
                                     // the caller binds another target set for each of two consecutive frames and fences its reads (frr_frame_fence)
    int frames_in_flight = 2;        // option frames_in_flight (1: one target set, everything on the caller's stream)
    DevBuf<Counters> cnt;
    FrameState fs;
    int cull = FRR_CULL_NONE;       // frr_set_cull: travels with every geometry pass issued from now on (Cmd::cull), like the uniforms
    GeomSet gset[2];
    BinSet bset[2];
    // cross-stream ordering: every workspace set has an event that fires when the latest tile kernel reading it is done (the second
    // stream waits for it before it overwrites a workspace that kernel reads), ev_bin[k & 3] when binning k is done
    Event ev_bin[4], ev_join;
    Event ev_keep[4];               // a predicated pass's stream behind the ctx's other streams, one event per stream (exec_geometry)
    uint64_t bin_serial = 0;
    // inputs the caller wrote on `stream` (a device-bound mesh) must be visible to the ctx's private streams: every bind
    // starts a new epoch, and a private stream waits for `stream` once per epoch before its next geometry pass
    uint32_t join_epoch = 1, joined_g = 0;   // (joined_g: gstream's; a frame stream's is FrameStream::joined)
    // command log since the last synchronisation point / frr_clear (finish(): replay)
    std::vector<Cmd> log;
    // shade_from_host (frr_shade_varyings_host, frr_shade_items_host): the device copies of the callers' buffers, one per logged command that reads one (Cmd::shade_in
    // is a view of it); freed whenever the log is (drop_log)
    std::vector<DevBuf<float>> shade_tmp;
    uint32_t next_seq = 1, epoch = 1;
    uint32_t replays = 0;           // replays since frr_clear (frr_stats.replays)
    bool in_replay = false;
    Counters hc;                    // host copy of the device counters as of the latest finish()
    uint32_t *host_bad = nullptr;   // host-visible word the device writes a failed command's number to (Counters::host_bad); hipHostMalloc, freed by frr_destroy
    uint32_t seen_bad = SEQ_NONE;   // its value when the host last looked
    // A draw cannot fail, whoever consumes its targets and however (stream order, frr_frame_fence, frr_sync): a raster pass whose
    // need of the work lists is not known to fit -- no pass with the same DrawSig has completed on the current lists -- is
    // VERIFIED before frr_raster returns: the host waits for the pass's binning launch (not for its tile kernel), looks at
    // host_bad, and repairs (finish(): grow + replay) if the pass or its geometry overflowed.  A proven pass is not waited for.
    ProvenSet proven;               // (frr_proof.h)
    uint64_t mesh_gen = 0;          // meshes registered so far (Mesh::gen)
    uint64_t tex_epoch = 0;         // frr_texture_upload calls so far (DrawSig: a user VS may sample a texture)
    uint64_t sync_epoch = 0;        // frr_sync calls so far (DrawSig of a device-bound mesh: rewritten in place behind one?)
    Event ev_verify;
    bool verify_pending = false;
    bool verify_pred = false;       // the pass being verified is predicated: verified every time, it never enters `proven`
    DrawSig verify_sig;
    // own targets handed out (frr_target_ptrs / frr_frame_fence): the frame that next renders into that set waits for what
    // the stream they were handed to holds by then (the caller's reads), see frr_clear
    bool exported[2] = {false, false};
    hipStream_t export_stream[2] = {nullptr, nullptr};
    Event ev_export;
    // frr_frame_wait: one event per stream handed in (recorded on it), pending until a target write issued after the latest
    // frr_frame_wait consumes them; every target write until then -- a deferred clear of an earlier frame or binding too --
    // waits for all of them.  Events are reused (wait_pool).
    struct FrameWait { hipStream_t stream; Event ev; };
    std::vector<FrameWait> waits;
    std::vector<Event> wait_pool;
    uint32_t wait_serial = 0;       // frr_frame_wait calls so far
    size_t fan_hint = 0;       // fan capacity asked for by a draw that overflowed
    int bin_g = 0;             // option bin_chunks: override the number of binning chunks (dev)
    uint32_t ent_slot_override = 0; // option tile_slot_records: per-tile slot of bins2 in records (tests of the overflow arena)
    bool clear_eager = false;
    bool bin_atomics = false;  // option bin_atomics: force the global-atomic binning fallback (tests)
    size_t bin_cap_init = 0;   // option bin_capacity: initial capacity of the (triangle, tile) lists in records (overflow / replay tests)
    size_t fan_cap_init = 0;   // option fan_capacity: initial fan capacity (the same)
    int clip_queue = -1;        // option clip_queue: 1 use the queue + k_geom_clip, 0 never, -1 when the latest counters read back
    bool clip_queue_auto = false; //   showed a block with more than CLIP_QUEUE_AT clipped inputs (results are the same either way)
    // binning workspace of the CSR fallback (one set: that path does not overlap)
    DevBuf<uint32_t> tile_counts, tile_offsets, tile_cursor;
    uint32_t max_tiles = 0;
    bool lds_attr_set = false;
    std::vector<Mesh> meshes;
    std::vector<Lines> lines;
    std::vector<Instances> instances;
    std::vector<Materials> materials;
    // frr_shade_items: what the material of an EMPTY texture slot samples (ShadeItemsArgs::zero_tex): one texel of zeros, so
    // that frr::sample_2d of such a material reads memory that exists; written once by frr_create
    DevBuf<uint8_t> zero_texel;
    uint64_t inst_gen = 0;          // instance tables registered so far (Instances::gen)
    std::vector<DrawList> lists;
    uint64_t list_gen = 0;          // draw lists uploaded so far (DrawList::gen)
    DevBuf<uint32_t> item_tmp;      // frr_geometry_item_ranges: the device side of its answer
    // draw_line order is resolved per pixel on a u32 plane of W * H (frr_lines.h), all-zero between commands: one per stream
    // that can carry target writes -- [0] `stream`, [1] / [2] the frame streams tstream[0] / tstream[1] -- because the line
    // commands of two frames in flight run beside each other.  Allocated and zeroed on first use.
    DevBuf<uint32_t> line_owner[3];
    uint32_t lines_chunk = 0;       // option lines_chunk (0: LINES_CHUNK)
    // frr_visible_pixels, frr_shade_items: the item boundaries of a command in flight, one table per stream that can carry one
    // (as line_owner); commands of one stream follow each other, and every one builds the table again
    DevBuf<uint32_t> vis_bounds[3];
    uint32_t visible_lds_bins = 0;  // option visible_lds_bins (0: VIS_LDS_BINS)
    // frr_query_boxes: the depth pyramid of a command in flight, one per stream that can carry one (as vis_bounds); every
    // command builds it again.  Sized by the window before the command is logged, so a replay never grows it.
    DevBuf<uint32_t> box_pyr[3];
    uint32_t box_bounds_chunks = 0; // option box_bounds_chunks: cap on the workgroups per mesh of k_box_bounds (0: 1,024; the tests' hook for its stride loop)
    // per lane of device tables: the latest wireframe reads its geometry pass's fan cursors, which the next pass IN THAT LANE
    // zeroes (geom_bookkeeping), whatever workspace set it writes; the other lane's frame shares nothing with it
    ReaderFence wire_reader[2];
    std::map<int, UserModule> user_modules;   // user shader id -> its code object loaded on this ctx's device
    Texture tex[FRR_MAX_TEXTURES];
    frr_uniforms uni;
    DevUniforms duni;
    bool count_frags = true;   // exact covered-fragment statistic (disables whole-triangle early-z)
    int raster_nw = 0;         // option raster_nw: force 3 / 4 / 6 / 8 / 16 waves per tile workgroup (dev)
    int raster_occ = 0;        // option raster_occ: force the 6- or 8-waves-per-SIMD build of the tile kernel (dev)
    bool raster_sweep = false; // option raster_sweep: brute-force tile kernel instead of the span kernel
    int tile_order = TILE_ORDER_FIXED;   // option tile_order: which block of the tile kernel takes which tile (frr_tile_order.h)
    uint64_t ordered_passes = 0;   // raster passes whose tile kernel took a built order (frr_tile_order_passes)
#ifdef FRR_DEBUG_COUNTERS
    DevBuf<unsigned long long> dbg_tiles;    // FRR_DEBUG_TILES: per-tile timeline of the latest tile kernel
#endif
    Event ev[16];             // frr_event_record (timing events)
    bool ev_set[16] = {};
    uint32_t prof_mask = 0;   // bit per KernelId
    std::vector<ProfRec> prof_pending;
    std::vector<Event> ev_pool;      // timing events of the profile, between uses
    uint32_t prof_period = 1;         // bracket only every prof_period-th launch of a kernel (frr_profile_set_period)
    uint32_t prof_seen[KID_COUNT] = {};
    double prof_ms[KID_COUNT] = {};
    uint32_t prof_n[KID_COUNT] = {};
    std::string err;
};

namespace {

int fail(frr_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    return code;
}
#define HIP_TRY(c, expr)                                                                                    \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return fail(c, FRR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
    } while (0)
int hip_rc(frr_ctx *c, hipError_t e) { return e == hipSuccess ? FRR_OK : fail(c, FRR_ERR_HIP, hipGetErrorString(e)); }
int nomem(frr_ctx *c, const char *what) { return fail(c, FRR_ERR_NOMEM, std::string("out of device memory: ") + what + ": " + hipGetErrorString(hipPeekAtLastError())); }

bool own_targets(const frr_ctx *c)
{
    const Bound &b = c->fs.bound;
    return b.color == c->own_color[b.tset] && b.depth == c->own_depth[b.tset] && b.tri_id == c->own_tri_id[b.tset];
}
// do consecutive frames (frr_clear) alternate between two streams / target sets / workspace sets / lanes?
bool frames_alternate(const frr_ctx *c) { return c->frames_in_flight == 2 && (own_targets(c) || c->bound_in_flight); }
// the stream of everything that touches the current frame targets: `stream`, or the current target set's c->tstream[tset]
hipStream_t tstream_of(const frr_ctx *c)
{
    const hipStream_t t = c->tstream[c->fs.bound.tset].st;
    if (own_targets(c)) return t && c->fs.bound.tset == 1 ? t : c->stream;
    return c->bound_in_flight && c->tstream[0].st && c->tstream[1].st ? t : c->stream;
}
// the stream of the latest geometry pass and of the binning that follows it: the second stream, or the targets' stream
hipStream_t gstream_of(const frr_ctx *c) { return c->fs.geom.on_g ? c->gstream : tstream_of(c); }
// do passes ever run beside each other on this ctx (workspace sets then carry events)?
bool multi_stream(const frr_ctx *c) { return c->g_used || c->tstream[0].st || c->tstream[1].st; }

// the ctx's own target set t (the second one is allocated on first use)
int ensure_own_set(frr_ctx *c, int t)
{
    const size_t npx = (size_t)c->W * c->H;
    const bool ok = (c->own_color[t] || c->own_color[t].reset(npx * 4) == hipSuccess) &&
                    (c->own_depth[t] || c->own_depth[t].reset(npx) == hipSuccess) &&
                    (c->own_tri_id[t] || c->own_tri_id[t].reset(npx) == hipSuccess);
    return ok ? FRR_OK : nomem(c, "frame targets");
}

// the logged commands are history: nothing replays them any more, so the buffers they alone read go too (hipFree waits for
// the device: a shade of a frame still in flight has read its copy by the time it is freed)
void drop_log(frr_ctx *c)
{
    c->log.clear();
    c->shade_tmp.clear();
}

// all streams idle
int drain(frr_ctx *c)
{
    for (hipStream_t st : {c->gstream, c->tstream[1].st, c->tstream[0].st, c->stream}) if (st) HIP_TRY(c, hipStreamSynchronize(st));
    for (FrameStream &t : c->tstream) t.dirty = t.xdirty = false;
    c->g_used = false;
    for (int i = 0; i < 2; ++i) c->gset[i].reader.pending = c->bset[i].reader.pending = false;
    for (ReaderFence &r : c->wire_reader) r.pending = false;
    return FRR_OK;
}
// a caller's stream waits for the ctx's frame streams: what is enqueued on it next sees every frame issued so far
int fence_stream(frr_ctx *c, hipStream_t st)
{
    const bool own = st == c->stream;
    if (!own && st != c->xfence) { c->xfence = st; for (FrameStream &t : c->tstream) t.xdirty = t.st != nullptr; }
    for (int i = 1; i >= 0; --i) {
        FrameStream &t = c->tstream[i];
        bool &unjoined = own ? t.dirty : t.xdirty;   // (set only while t.st exists)
        if (unjoined) {
            HIP_TRY(c, hipEventRecord(t.ev, t.st));
            HIP_TRY(c, hipStreamWaitEvent(st, t.ev, 0));
        }
        unjoined = false;
    }
    if (!own && !(c->bound_in_flight && c->tstream[0].st)) {   // (frames may have run on the ctx's stream itself)
        HIP_TRY(c, hipEventRecord(c->ev_join, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(st, c->ev_join, 0));
    }
    return FRR_OK;
}
int join_tile_streams(frr_ctx *c) { return fence_stream(c, c->stream); }

// a workspace buffer of at least `need` elements; *fresh: it is new memory, what the old one held is gone
template <typename T> int ensure(frr_ctx *c, DevBuf<T> &b, size_t need, bool *fresh = nullptr)
{
    const bool grow = need > b.cap() || !b;
    if (fresh) *fresh = grow;
    if (!grow) return FRR_OK;
    if (b) { int rc = drain(c); if (rc != FRR_OK) return rc; HIP_TRY(c, b.release()); }   // (the device may still be reading it)
    return b.reset(need) == hipSuccess ? FRR_OK : nomem(c, "workspace");
}
// a fresh buffer that holds `bytes` of host memory, copied on c->stream; wait: the host waits for it (false: the call's next upload will)
template <typename T> int upload(frr_ctx *c, DevBuf<T> &out, const void *host, size_t bytes, const char *what, bool wait = true)
{
    DevBuf<T> b;
    if (b.reset((bytes + sizeof(T) - 1) / sizeof(T)) != hipSuccess) return nomem(c, what);
    hipError_t e = bytes ? hipMemcpyAsync(b.get(), host, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    if (e == hipSuccess && wait) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) out = std::move(b);   // (only now: a failed upload leaves what `out` held)
    return hip_rc(c, e);
}
// The first bad element of a list in the caller's device memory, 0xFFFFFFFF if none: launch(cell) starts one reduction over the
// list on the caller's stream -- behind whatever wrote the list -- and the host waits for it (binding is a set-up call).
template <typename Launch> int first_bad_on_device(frr_ctx *c, uint32_t *bad, Launch launch)
{
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<uint32_t> cell;
    if (cell.reset(4) != hipSuccess) return nomem(c, "check cell");
    *bad = 0xFFFFFFFFu;
    hipError_t e = hipMemcpyAsync(cell.get(), bad, sizeof *bad, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch(cell.get()); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(bad, cell.get(), sizeof *bad, hipMemcpyDeviceToHost, c->stream);
    return hip_rc(c, e == hipSuccess ? hipStreamSynchronize(c->stream) : e);
}

// ---- cross-stream ordering (no-ops when everything runs on one stream) ----------------------------------------------
// the second stream waits until the latest tile kernel that reads a workspace set is done
int gstream_wait_readers(frr_ctx *c, ReaderFence &r)
{
    if (!r.pending) return FRR_OK;
    r.pending = false;
    if (r.stream == gstream_of(c)) return FRR_OK;   // same stream: already in order
    // (the event may not have been recorded at the launch: then now, after whatever else the reader's stream has been given
    // since -- more than needed, and right for the rare change of pattern this serves)
    if (!r.recorded) HIP_TRY(c, hipEventRecord(r.ev, r.stream));
    HIP_TRY(c, hipStreamWaitEvent(gstream_of(c), r.ev, 0));
    return FRR_OK;
}
// the stream of the geometry pass about to be issued waits for everything the caller's stream holds so far (mesh data
// written by the caller before it bound the mesh), once per bind
int gstream_join(frr_ctx *c)
{
    hipStream_t st = gstream_of(c);
    if (st == c->stream) return FRR_OK;
    uint32_t &joined = st == c->gstream ? c->joined_g : c->tstream[c->fs.bound.tset].joined;   // (tstream_of)
    if (joined == c->join_epoch) return FRR_OK;
    HIP_TRY(c, hipEventRecord(c->ev_join, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(st, c->ev_join, 0));
    joined = c->join_epoch;
    return FRR_OK;
}
// the tile stream waits for what the second stream holds so far (binning -> tile kernel)
int tstream_wait_gstream(frr_ctx *c)
{
    if (gstream_of(c) == tstream_of(c)) return FRR_OK;
    hipEvent_t e = c->ev_bin[++c->bin_serial & 3];
    HIP_TRY(c, hipEventRecord(e, gstream_of(c)));
    HIP_TRY(c, hipStreamWaitEvent(tstream_of(c), e, 0));
    return FRR_OK;
}
// a tile kernel has just been launched on `ts`: the workspace sets it reads are busy until it is done
int tile_launched(frr_ctx *c, hipStream_t ts, GeomSet &gs, BinSet &bs)
{
    if (!multi_stream(c)) return FRR_OK;   // everything has run on one stream so far
    // Frames in flight give every frame stream its own workspace sets: the next writer of a set is on the reader's stream, and
    // no event is needed (should the pattern change, gstream_wait_readers records one late).  With geometry + binning on the
    // second stream the event is what lets that stream run beside the NEXT tile kernel: recorded right here.
    const bool eager = c->g_used;
    for (ReaderFence *r : {&gs.reader, &bs.reader}) {
        r->pending = true; r->stream = ts; r->recorded = eager;
        if (eager) HIP_TRY(c, hipEventRecord(r->ev, ts));
    }
    return FRR_OK;
}

// e: an event out of a pool of spare ones, or a new one (empty, and the error, if it cannot be created)
hipError_t pooled_event(std::vector<Event> &pool, bool timing, Event &e)
{
    if (pool.empty()) return e.create(timing);
    e = std::move(pool.back()); pool.pop_back();
    return hipSuccess;
}
struct ProfScope {
    frr_ctx *c; int kid; hipStream_t st; Event a;
    ProfScope(frr_ctx *c_, int kid_, hipStream_t st_) : c(c_), kid(kid_), st(st_)
    {
        if ((c->prof_mask & (1u << kid)) && (c->prof_seen[kid]++ % c->prof_period) == 0) {
            (void)pooled_event(c->ev_pool, true, a);   // (empty: the sample is dropped)
            if (a && hipEventRecord(a, st) != hipSuccess) c->ev_pool.push_back(std::move(a));
        }
    }
    ~ProfScope()
    {
        // a sample whose events could not be created or recorded is dropped (frr_profile_get then reports fewer launches)
        if (!a) return;
        Event b;
        (void)pooled_event(c->ev_pool, true, b);
        if (b && hipEventRecord(b, st) == hipSuccess) { c->prof_pending.push_back({kid, std::move(a), std::move(b)}); return; }
        c->ev_pool.push_back(std::move(a));
        if (b) c->ev_pool.push_back(std::move(b));
    }
};
void prof_collect(frr_ctx *c)
{
    if (c->prof_pending.empty()) return;
    (void)drain(c);
    for (auto &r : c->prof_pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { c->prof_ms[r.kid] += ms; c->prof_n[r.kid]++; }
        c->ev_pool.push_back(std::move(r.a)); c->ev_pool.push_back(std::move(r.b));
    }
    c->prof_pending.clear();
}

// glam Mat4*Mat4 = columns (self * rhs.col_j), Mat4*Vec4 = ((c0*x + c1*y) + c2*z) + c3*w
void h_mat4_mul(const float *a, const float *b, float *out)
{
    float t[16];
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r)
            t[4 * c + r] = ((a[r] * b[4 * c] + a[4 + r] * b[4 * c + 1]) + a[8 + r] * b[4 * c + 2]) + a[12 + r] * b[4 * c + 3];
    memcpy(out, t, sizeof t);
}

void refresh_dev_uniforms(frr_ctx *c)
{
    DevUniforms &d = c->duni;
    float pv[16];
    h_mat4_mul(c->uni.proj, c->uni.view, pv);   // proj * view * model is left-associative (phong.rs:119)
    h_mat4_mul(pv, c->uni.model, d.mvp);
    memcpy(d.model, c->uni.model, sizeof d.model);
    memcpy(d.view_pos, c->uni.view_pos, sizeof d.view_pos);
    memcpy(d.light_pos, c->uni.light_pos, sizeof d.light_pos);
    memcpy(d.light_color, c->uni.light_color, sizeof d.light_color);
    d.ambient_strength = c->uni.ambient_strength;
    d.specular_strength = c->uni.specular_strength;
    memcpy(d.flat_color, c->uni.flat_color, sizeof d.flat_color);
    int s = c->uni.texture_slot;
    if (s >= 0 && s < FRR_MAX_TEXTURES) { d.tex = c->tex[s].dev; d.tex_w = c->tex[s].w; d.tex_h = c->tex[s].h; }
    else { d.tex = nullptr; d.tex_w = d.tex_h = 0; }
    for (int k = 0; k < FRR_MAX_TEXTURES; ++k) { d.slot_tex[k] = c->tex[k].dev; d.slot_w[k] = c->tex[k].w; d.slot_h[k] = c->tex[k].h; }
}

// Tile rows [t0, t1) of rank `rank` in the blocked layout: the first tiles_y % world ranks own one row more than the
// others, so that no rank of world <= tiles_y is left without rows (34 rows over 8 ranks: 5,5,4,4,4,4,4,4)
void blocked_rows(int tiles_y, int rank, int world, int *t0, int *t1)
{
    const int q = tiles_y / world, r = tiles_y % world;
    *t0 = rank * q + std::min(rank, r);
    *t1 = *t0 + q + (rank < r ? 1 : 0);
}

// The ctx's tile-row ownership over `tiles_y` tile rows.  `blocked` is set on a real partition only (world > 1): without one every
// reader (owns_tile_row -- so k_clear_unowned_rows too --, local_tile_row, tri_rows_owned) answers from `world <= 1` before the layout.
RowOwner row_owner(const FrameState &f, int tiles_y)
{
    const Bound &b = f.bound;
    RowOwner o = {b.rank, b.world, (b.part_blocked && b.world > 1) ? 1 : 0, 0, 0};
    if (o.blocked) blocked_rows(tiles_y, b.rank, b.world, &o.brow0, &o.brow1);
    return o;
}

// the code object of user shader `id` on this ctx's device
int user_module(frr_ctx *c, int id, const UserModule **out)
{
    auto it = c->user_modules.find(id);
    if (it != c->user_modules.end()) { *out = &it->second; return FRR_OK; }
    const UserShader *us = user_shader(id);
    if (!us) return fail(c, FRR_ERR_INVALID, "unknown shader id");
    UserModule m;
    HIP_TRY(c, hipModuleLoadData(&m.mod, us->code.data()));
    HIP_TRY(c, hipModuleGetFunction(&m.geom, m.mod, us->geom.c_str()));
    HIP_TRY(c, hipModuleGetFunction(&m.clip, m.mod, us->clip.c_str()));
    HIP_TRY(c, hipModuleGetFunction(&m.geom_idx, m.mod, us->geom_idx.c_str()));
    HIP_TRY(c, hipModuleGetFunction(&m.clip_idx, m.mod, us->clip_idx.c_str()));
    for (int idx = 0; idx < 2; ++idx) {
        HIP_TRY(c, hipModuleGetFunction(&m.geom_inst[idx], m.mod, us->geom_inst[idx].c_str()));
        HIP_TRY(c, hipModuleGetFunction(&m.clip_inst[idx], m.mod, us->clip_inst[idx].c_str()));
    }
    HIP_TRY(c, hipModuleGetFunction(&m.geom_list, m.mod, us->geom_list.c_str()));
    HIP_TRY(c, hipModuleGetFunction(&m.clip_list, m.mod, us->clip_list.c_str()));
    HIP_TRY(c, hipModuleGetFunction(&m.sweep, m.mod, us->sweep.c_str()));
    HIP_TRY(c, hipModuleGetFunction(&m.entries, m.mod, us->entries.c_str()));
    for (int cnt = 0; cnt < 2; ++cnt)
        for (int sh = 0; sh < 6; ++sh) HIP_TRY(c, hipModuleGetFunction(&m.span[cnt][sh], m.mod, us->span[cnt][sh].c_str()));
    for (int vec = 0; vec < 2; ++vec)
        if (!us->shade[vec].empty()) {   // ([1]: only where K is a multiple of 4)
            HIP_TRY(c, hipModuleGetFunction(&m.shade[vec], m.mod, us->shade[vec].c_str()));
            HIP_TRY(c, hipModuleGetFunction(&m.shade_items[vec], m.mod, us->shade_items[vec].c_str()));
        }
    *out = &(c->user_modules[id] = m);
    return FRR_OK;
}

constexpr uint32_t kClipGrid = 2048;      // workgroups of k_geom_clip (four wavefronts each, one triangle per wavefront and step)

// (IDX, an indexed mesh, is a template flag and not a null test in the kernels: the instantiations for expanded meshes keep
// their code; so is INST, an instanced pass, and LIST, a list pass, which takes INST's matrices and branches on the item for IDX)
template <int VS, bool IDX, bool INST, bool LIST = false> void launch_geometry_as(frr_ctx *c, GeomArgs &g, uint32_t nblocks, const DevUniforms &du)
{
    hipStream_t st = gstream_of(c);
    hipLaunchKernelGGL((k_geom_single<VS, IDX, INST, LIST>), dim3(nblocks), dim3(GEOM_BLOCK), 0, st, g, du);
    if (g.use_clipq) hipLaunchKernelGGL((k_geom_clip<VS, IDX, INST, LIST>), dim3(std::min<uint32_t>(kClipGrid, nblocks * 4u)), dim3(GEOM_BLOCK), 0, st, g, du);
}

template <int VS> void launch_geometry(frr_ctx *c, GeomArgs &g, uint32_t nblocks, const DevUniforms &du)
{
    if (g.items) launch_geometry_as<VS, false, true, true>(c, g, nblocks, du);
    else if (g.inst) {
        if (g.idx) launch_geometry_as<VS, true, true>(c, g, nblocks, du);
        else launch_geometry_as<VS, false, true>(c, g, nblocks, du);
    } else if (g.idx) launch_geometry_as<VS, true, false>(c, g, nblocks, du);
    else launch_geometry_as<VS, false, false>(c, g, nblocks, du);
}

// the geometry kernel for the VS of the mesh; models: the table of an instanced pass (or the matrices of a list's items), whose matrices (GeomArgs::inst = pv * model
// and model, per instance) are filled first -- on the pass's stream and inside the command, so a replay fills them again
// keep, min_value: a predicated list pass, whose keep table (GeomArgs::keep) is filled the same way, from the caller's buffer
void launch_geometry_vs(frr_ctx *c, GeomArgs &g, uint32_t nblocks, int vs, const DevUniforms &du, const UserModule *um, const float *models, const float *pv,
                        const uint32_t *keep, uint32_t min_value)
{
    hipStream_t st = gstream_of(c);
    ProfScope p(c, KID_GEOM, st);
    if (g.keep) hipLaunchKernelGGL(k_item_keep, dim3((g.ninst + 255u) / 256u), dim3(256), 0, st, keep, min_value, const_cast<uint32_t *>(g.keep), g.ninst);
    if (g.inst) {
        Mat4Arg m;
        memcpy(m.m, pv, sizeof m.m);
        hipLaunchKernelGGL(k_instance_mvp, dim3((g.ninst * 4u + 255u) / 256u), dim3(256), 0, st, models, m, const_cast<float *>(g.inst), g.ninst);
    }
    if (um) {   // a user shader: the same kernels, compiled with the user's functions (frr_shader_register)
        DevUniforms d = du;
        void *args[] = {&g, &d};
        const hipFunction_t geom = g.items ? um->geom_list : g.inst ? um->geom_inst[g.idx ? 1 : 0] : g.idx ? um->geom_idx : um->geom;
        const hipFunction_t clip = g.items ? um->clip_list : g.inst ? um->clip_inst[g.idx ? 1 : 0] : g.idx ? um->clip_idx : um->clip;
        (void)hipModuleLaunchKernel(geom, nblocks, 1, 1, GEOM_BLOCK, 1, 1, 0, st, args, nullptr);
        if (g.use_clipq) (void)hipModuleLaunchKernel(clip, std::min<uint32_t>(kClipGrid, nblocks * 4u), 1, 1, GEOM_BLOCK, 1, 1, 0, st, args, nullptr);
        return;
    }
    switch (vs) {
    case FRR_VS_CLIP: launch_geometry<FRR_VS_CLIP>(c, g, nblocks, du); break;
    case FRR_VS_CLIP_COLOR: launch_geometry<FRR_VS_CLIP_COLOR>(c, g, nblocks, du); break;
    case FRR_VS_PHONG: launch_geometry<FRR_VS_PHONG>(c, g, nblocks, du); break;
    case FRR_VS_GOURAUD: launch_geometry<FRR_VS_GOURAUD>(c, g, nblocks, du); break;
    }
}
// the latest geometry pass's block sums -> prefix (+ n_emit, the fan-capacity flag), if no binning launch has done it
int scan_now(frr_ctx *c)
{
    FrameState &f = c->fs;
    if (!f.geom.scan_pending) return FRR_OK;
    hipStream_t st = gstream_of(c);
    { ProfScope p(c, KID_GEOM_SCAN, st); hipLaunchKernelGGL(k_geom_scan, dim3(1), dim3(1024), 0, st, c->gset[f.geom.set].block_sums, c->gset[f.geom.set].block_prefix, f.geom.nblocks, c->cnt, f.lane, f.gpar(), f.geom.fan_cap, f.geom.seq, c->epoch); }
    HIP_TRY(c, hipGetLastError());
    f.geom.scan_pending = false;
    return FRR_OK;
}

// Shape of the tile kernel's workgroups for `grid` tiles: NW waves per tile (and the waves per SIMD its registers are
// budgeted for).  Measured on the 1080p / 4096^2 / 4K frames (profiles/, tools/exp_shapes.py): a CU is issue-bound with
// six 4-wave workgroups, so budgeting registers for eight buys nothing; wider workgroups shorten a tile's chain and win
// when the tiles do not fill the chip (a partitioned rank, a small window); three waves per tile win when there are
// many lightly loaded tiles of a depth-only draw (about 120 records each on the 4096^2 frame: four waves would cull 30
// records apiece); shaded draws keep four (the resolve is most of their work: 55 vs 88 us on the 69k-triangle sphere).
struct SpanShape { int nw, occ; };
SpanShape span_shape(const frr_ctx *c, uint32_t grid, uint64_t ntris, int ps_id)
{
    if (c->raster_nw || c->raster_occ)                   // options raster_nw / raster_occ (tests, tools)
        for (const auto &k : kSpanShapes)
            if ((!c->raster_nw || k[0] == c->raster_nw) && (!c->raster_occ || k[1] == c->raster_occ)) return {k[0], k[1]};
    if (grid <= 256u) return {16, 4};
    if (grid <= 768u) return {8, 6};
    if (ps_id == FRR_PS_DEPTH && grid > 1536u && ntris * 2u <= 192ull * grid) return {LIGHT_NW, 6};
    return {4, 6};
}

template <int K, int PS> void launch_raster(frr_ctx *c, hipStream_t ts, const RasterArgs &a, uint32_t grid, const SpanShape sh, const DevUniforms &du, bool count_frags, int win_safe)
{
    ProfScope p(c, KID_RASTER, ts);
    if (c->raster_sweep) {
        hipLaunchKernelGGL((k_raster<K, PS>), dim3(grid), dim3(256), 0, ts, a, du);
    } else {
        auto go = [&](auto count_tag, auto nw_tag, auto occ_tag) {
            constexpr bool CNT = decltype(count_tag)::value;
            constexpr int NWV = decltype(nw_tag)::value, OCCV = decltype(occ_tag)::value;
            hipLaunchKernelGGL((k_raster_span<K, PS, CNT, NWV, OCCV>), dim3(grid), dim3(NWV * 64), 0, ts, a, du, win_safe);
        };
        auto go_nw = [&](auto count_tag) {
            if (sh.nw == LIGHT_NW) go(count_tag, std::integral_constant<int, LIGHT_NW>{}, std::integral_constant<int, 6>{});
            else if (sh.nw == 4 && sh.occ == 8) go(count_tag, std::integral_constant<int, 4>{}, std::integral_constant<int, 8>{});
            else if (sh.nw == 4) go(count_tag, std::integral_constant<int, 4>{}, std::integral_constant<int, 6>{});
            else if (sh.nw == 6) go(count_tag, std::integral_constant<int, 6>{}, std::integral_constant<int, 6>{});
            else if (sh.nw == 8) go(count_tag, std::integral_constant<int, 8>{}, std::integral_constant<int, 6>{});
            else go(count_tag, std::integral_constant<int, 16>{}, std::integral_constant<int, 4>{});
        };
        if (count_frags) go_nw(std::true_type{}); else go_nw(std::false_type{});
    }
}

// `ts` (tstream_of) has been given work: a frame stream is dirty until fence_stream joins it
void frame_stream_dirty(frr_ctx *c, hipStream_t ts)
{
    if (ts != c->stream) c->tstream[c->fs.bound.tset].dirty = c->tstream[c->fs.bound.tset].xdirty = true;
}
// which of the buffers kept per stream that can carry target work (frr_ctx::line_owner, vis_bounds) goes with `ts`
int stream_slot(const frr_ctx *c, hipStream_t ts) { return ts == c->stream ? 0 : ts == c->tstream[0].st ? 1 : 2; }
// Every launch that writes the frame targets goes on the stream this returns (*ts, the targets' stream).  The write follows
// every stream of a pending frr_frame_wait, and its stream, if a frame stream, is dirty until fence_stream joins it.
// `consume`: the write was issued after the latest frr_frame_wait (the one the waits are for), so later writes follow it
// and need not wait themselves.
int target_write(frr_ctx *c, bool consume, hipStream_t *ts)
{
    *ts = tstream_of(c);
    frame_stream_dirty(c, *ts);
    for (const frr_ctx::FrameWait &w : c->waits) HIP_TRY(c, hipStreamWaitEvent(*ts, w.ev, 0));
    if (consume) {
        for (frr_ctx::FrameWait &w : c->waits) c->wait_pool.push_back(std::move(w.ev));
        c->waits.clear();
    }
    return FRR_OK;
}

// the clear itself (k_clear), on the targets' stream; `issued_after_waits`: the frr_clear came after the latest frr_frame_wait
int clear_now(frr_ctx *c, uint32_t packed, float depth, bool issued_after_waits)
{
    const FrameState &f = c->fs;
    const uint32_t n = c->W * c->H, n4 = n / 4;
    hipStream_t ts;
    { int rc = target_write(c, issued_after_waits, &ts); if (rc != FRR_OK) return rc; }
    {
        ProfScope p(c, KID_CLEAR, ts);
        uint32_t grid = std::min<uint32_t>((n4 + 255) / 256, 2048);
        hipLaunchKernelGGL(k_clear, dim3(grid ? grid : 1), dim3(256), 0, ts, (uint4 *)f.bound.color, (uint4 *)f.bound.depth,
                           (uint4 *)f.bound.tri_id, n4, packed, depth);
        if (n4 * 4 < n)
            hipLaunchKernelGGL(k_clear_tail, dim3(1), dim3(64), 0, ts, (uint32_t *)f.bound.color, (uint32_t *)f.bound.depth,
                               f.bound.tri_id, n4 * 4, n, packed, depth);
    }
    HIP_TRY(c, hipGetLastError());
    return FRR_OK;
}

// bring the targets to the state the API promises (a pending frr_clear; rows a fused clear of a partitioned ctx skipped)
int settle_targets(frr_ctx *c)
{
    FrameState &f = c->fs;
    if (f.clear.pending) {
        int rc = clear_now(c, f.clear.rgba, f.clear.depth, f.clear.wait_serial == c->wait_serial);
        if (rc != FRR_OK) return rc;
        f.clear.pending = f.clear.unowned_debt = false;
    } else if (f.clear.unowned_debt) {
        const RowOwner own = row_owner(f, f.clear.debt_tiles_y);
        // (the rest of a clear issued with an earlier draw: it follows the pending waits, the next frame's writes consume them)
        hipStream_t ts;
        { int rc = target_write(c, false, &ts); if (rc != FRR_OK) return rc; }
        hipLaunchKernelGGL(k_clear_unowned_rows, dim3(c->H), dim3(256), 0, ts, (uint32_t *)f.bound.color, (uint32_t *)f.bound.depth,
                           f.bound.tri_id, c->W, c->H, own, f.clear.rgba, f.clear.depth);
        HIP_TRY(c, hipGetLastError());
        f.clear.unowned_debt = false;
    }
    return FRR_OK;
}
// ... and the tables of the latest geometry pass (called by everything that looks at either)
int settle(frr_ctx *c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    { int rcs = scan_now(c); if (rcs != FRR_OK) return rcs; }   // n_emit of the latest pass (statistics, setup read-back)
    return settle_targets(c);
}

// ---- what the commands that own no device table share (Cmd::owns_table) ---------------------------------------------
// Each runs behind a geometry pass, cannot fail on the device, and is replayed by running it again in its place: behind a
// failed command it writes nothing (seq_cancelled).  Two traits say how it is ordered.  reads_pass: it reads the tables of
// the latest geometry pass, on the device (no host wait).  writes_target: it writes a frame target.  An executor calls
// cmd_settle and cmd_stream, launches on the stream it was given, and calls cmd_done; its host-only steps that can refuse
// stand where they stood among these.

// What the command looks at is there: n_emit and the block prefix of the pass (a fan space that was too small is flagged
// here, before the tables are read: the command is then cancelled, and replayed), and the targets behind a pending frr_clear.
int cmd_settle(frr_ctx *c, bool reads_pass)
{
    int rc;
    if (reads_pass && (rc = scan_now(c)) != FRR_OK) return rc;
    return c->fs.clear.pending ? settle_targets(c) : FRR_OK;
}
// *ts: the stream its launches go on, which is the targets' stream.  A reader follows the pass's geometry there, as a tile
// kernel does.  A writer goes through target_write: it follows the streams of pending frr_frame_wait calls and, issued by
// the caller rather than by a replay, consumes them.  A command that writes no target has no business with those events
// (the caller's buffer is fenced like a target); it takes the same stream and, if that is a frame stream, leaves it dirty.
int cmd_stream(frr_ctx *c, bool reads_pass, bool writes_target, hipStream_t *ts)
{
    int rc;
    if (reads_pass && (rc = tstream_wait_gstream(c)) != FRR_OK) return rc;
    if (writes_target) return target_write(c, !c->in_replay, ts);
    *ts = tstream_of(c);
    frame_stream_dirty(c, *ts);
    return FRR_OK;
}
// The launches are on `ts`.  A reader has read the pass's tables there: the next pass in this lane, which zeroes the fan
// cursors and may overwrite the workspace, waits for it (frr_ctx::wire_reader), and finish() finds the tables it read in cmd.
void cmd_done(frr_ctx *c, Cmd &cmd, bool reads_pass, hipStream_t ts)
{
    const FrameState &f = c->fs;
    cmd.lane = f.lane;
    if (!reads_pass) return;
    ReaderFence &wr = c->wire_reader[f.lane];
    wr.pending = true; wr.stream = ts; wr.recorded = false;
    cmd.par = f.gpar(); cmd.set = f.geom.set;
}

// ---- the two commands ------------------------------------------------------------------------------------------------
// Loop A (phong.rs:321-331) over the mesh: one geometry pass.  Nothing of the host state is committed before the last
// step that can fail.  An instanced pass (cmd.inst >= 0) is the loop of phong.rs:319-331 over the objects around it as
// well: its inputs are the (instance, triangle) pairs in that order, and every list below is sized by their number.
int exec_geometry(frr_ctx *c, Cmd &cmd)
{
    FrameState &f = c->fs;
    // A list pass (cmd.list >= 0) is that loop over objects with a mesh of its own per object: its inputs are the items'
    // triangles one after the other, and it reads the list's snapshot, never frr_ctx::meshes.
    const DrawList *const dl = cmd.list >= 0 ? &c->lists[cmd.list] : nullptr;
    static const Mesh no_mesh;
    const Mesh &m = dl ? no_mesh : c->meshes[cmd.mesh];
    const Instances *const it = cmd.inst >= 0 ? &c->instances[cmd.inst] : nullptr;
    const int vs = dl ? dl->vs : m.vs;
    const int K = frr_vs_num_varyings(vs);
    const uint64_t nt = dl ? dl->total : it ? m.ntris * it->n : m.ntris;   // (below 2^27: frr_geometry_instanced, frr_drawlist_upload)
    const uint64_t nmat = dl ? dl->n : it ? it->n : 0;   // rows of the pass's matrix table
    const int par = f.gpar() ^ 1;
    // Beside the previous pass's tile kernel (second stream, the other workspace set) or after it (the targets' stream,
    // set 0: one set stays hot in the 256 MB Infinity Cache -- two sets of the 1M-triangle frame do not, which costs its
    // tile kernel 4 us).  Measured (profiles/r03_overlap_modes.txt): running beside pays for passes with varyings, whose
    // tile kernel spends long stretches shading (4K textured frame -6 %, a rank of 8 of it -10 %), not for depth-only ones.
    const bool fif2 = frames_alternate(c);   // consecutive frames already run beside each other, on two streams (frr_clear)
    const bool on_g = !fif2 && (c->overlap == 1 || (c->overlap == 2 && K > 0));
    const int si = on_g ? (f.geom.set ^ 1) : (fif2 ? f.bound.tset : 0);
    GeomSet &S = c->gset[si];
    int rc;
    const UserModule *um = nullptr;
    if (vs >= FRR_SHADER_USER_BASE && (rc = user_module(c, vs, &um)) != FRR_OK) return rc;
    // fan space: clipped inputs are the ones that straddle a frustum plane, usually few; room for as many fan triangles
    // as there are inputs (+ 4096) to start with, grown on demand (the pass then fails on the device and finish() replays
    // it with more) up to the worst case of 19 per input (small meshes get their worst case outright: 2^20 slots are cheap) ...
    const uint32_t nblocks = (uint32_t)((nt + GEOM_BLOCK - 1) / GEOM_BLOCK);
    // ... in FAN_REGIONS regions (block b allocates in region b % FAN_REGIONS: frr_device.h); a region never needs more
    // than 19 slots for every input of the blocks that use it
    const uint64_t region_worst = (uint64_t)FRR_MAX_OUT_TRIS * GEOM_BLOCK * ((nblocks + FAN_REGIONS - 1) / FAN_REGIONS);
    uint64_t first_guess = std::max<uint64_t>((nt + 4096 + FAN_REGIONS - 1) / FAN_REGIONS, std::min<uint64_t>(region_worst, (1u << 20) / FAN_REGIONS));
    if (c->fan_cap_init) first_guess = (c->fan_cap_init + FAN_REGIONS - 1) / FAN_REGIONS;   // option fan_capacity (tests of the replay)
    uint64_t region = std::max<uint64_t>(first_guess, (c->fan_hint + FAN_REGIONS - 1) / FAN_REGIONS);
    region = std::max<uint64_t>(std::min<uint64_t>(region, region_worst), 1);
    uint64_t fan_cap = region * FAN_REGIONS;
    if (nt + fan_cap > 0xFFFFFFF0ull) fan_cap = (0xFFFFFFF0ull - nt) / FAN_REGIONS * FAN_REGIONS;
    const size_t slots = (size_t)(nt + fan_cap);
    if ((rc = ensure(c, S.block_sums, (size_t)nblocks + 1)) != FRR_OK) return rc;
    if ((rc = ensure(c, S.block_prefix, (size_t)nblocks + 1)) != FRR_OK) return rc;
    if ((rc = ensure(c, S.tinfo, (size_t)std::max<uint64_t>(nt, 1))) != FRR_OK) return rc;
    if ((rc = ensure(c, S.fanbase, (size_t)std::max<uint64_t>(nt, 1))) != FRR_OK) return rc;
    if ((rc = ensure(c, S.fan_okey, (size_t)std::max<uint64_t>(fan_cap, 1))) != FRR_OK) return rc;
    if ((rc = ensure(c, S.recs, std::max<size_t>(slots, 1024))) != FRR_OK) return rc;
    if ((rc = ensure(c, S.pbox, S.recs.cap())) != FRR_OK) return rc;
    if ((rc = ensure(c, S.bcount, (size_t)nblocks + 1)) != FRR_OK) return rc;
    if (K > 0 && (rc = ensure(c, S.vary, S.recs.cap() * 3 * std::max(K, 8) /* (K <= 8 in the shader table) */)) != FRR_OK) return rc;
    const bool use_clipq = nt > 0 && (c->clip_queue > 0 || (c->clip_queue < 0 && c->clip_queue_auto));
    if (use_clipq && (rc = ensure(c, S.clipq, (size_t)nt)) != FRR_OK) return rc;
    if (nmat && nt > 0 && (rc = ensure(c, S.inst_tab, (size_t)nmat * 32)) != FRR_OK) return rc;
    const bool keep_tab = cmd.pred && nmat && nt > 0;
    if (keep_tab && (rc = ensure(c, S.keep_tab, (size_t)nmat)) != FRR_OK) return rc;
    if (on_g && !c->gstream) {
        // created on first use: a process maps its HIP streams onto a handful of hardware queues, and two streams that
        // share one run nothing beside each other -- a ctx that never needs this stream does not take a queue for it
        HIP_TRY(c, acquire_stream(c->device, &c->gstream));
    }
    if (on_g != f.geom.on_g) {
        // this pass changes streams: it follows the previous pass's geometry + binning (tri_base, fan cursors)
        hipEvent_t e = c->ev_bin[++c->bin_serial & 3];
        HIP_TRY(c, hipEventRecord(e, gstream_of(c)));
        HIP_TRY(c, hipStreamWaitEvent(on_g ? c->gstream : tstream_of(c), e, 0));
    }
    f.geom.on_g = on_g;
    if (on_g) c->g_used = true;
    // second stream: after whatever the caller's stream holds that this pass may read (first use), and after the tile
    // kernel that last read this workspace
    if ((rc = gstream_join(c)) != FRR_OK) return rc;
    if ((rc = gstream_wait_readers(c, S.reader)) != FRR_OK) return rc;
    if ((rc = gstream_wait_readers(c, c->wire_reader[f.lane])) != FRR_OK) return rc;
    if (keep_tab) {
        // The keep buffer is read on this pass's stream, behind every command issued on this ctx so far -- whichever of its
        // streams that ran on: the frr_visible_pixels of the previous frame is the intended writer -- and behind the streams
        // of pending frr_frame_wait calls (a caller that wrote the mask on a stream of its own).  Events only: no host wait.
        // (The waits stay pending: the pass's target write consumes them.)
        hipStream_t gs = gstream_of(c);
        const hipStream_t others[4] = {c->stream, c->tstream[0].st, c->tstream[1].st, c->gstream};
        for (int k = 0; k < 4; ++k) {
            if (!others[k] || others[k] == gs) continue;
            HIP_TRY(c, hipEventRecord(c->ev_keep[k], others[k]));
            HIP_TRY(c, hipStreamWaitEvent(gs, c->ev_keep[k], 0));
        }
        for (const frr_ctx::FrameWait &w : c->waits) HIP_TRY(c, hipStreamWaitEvent(gs, w.ev, 0));
    }
    GeomArgs g;
    g.in = m.dev; g.idx = m.idx; g.nverts = (uint32_t)m.nverts; g.ntris = (uint32_t)nt; g.width = c->W; g.height = c->H;
    g.fan_cap = (uint32_t)fan_cap;
    g.seq = cmd.seq; g.epoch = c->epoch; g.frame_no = f.frame_no;
    const RowOwner own = row_owner(f, (int)(((int64_t)cmd.fy1 - cmd.fy0 + TILE - 1) / TILE));
    g.part_rank = f.bound.rank; g.part_world = cmd.filter ? f.bound.world : 1; g.part_y0 = cmd.fy0; g.part_y1 = cmd.fy1;
    g.part_blocked = own.blocked; g.part_brow0 = own.brow0; g.part_brow1 = own.brow1;
    g.gpar = par; g.lane = f.lane;
    g.block_sums = S.block_sums; g.block_prefix = S.block_prefix; g.tinfo = S.tinfo; g.fanbase = S.fanbase; g.fan_okey = S.fan_okey;
    g.recs = S.recs; g.vary = S.vary; g.pbox = S.pbox; g.cnt = c->cnt;
    g.clipq = S.clipq; g.use_clipq = use_clipq ? 1 : 0;
    g.bcount = S.bcount;
    g.inst = nmat && nt > 0 ? S.inst_tab.get() : nullptr; g.ntris_mesh = (uint32_t)m.ntris; g.ninst = dl || it ? (uint32_t)nmat : 1u;
    g.items = dl && nt > 0 ? dl->rows.get() : nullptr; g.item_first = dl ? dl->first.get() : nullptr; g.item_ntris = dl ? dl->first.get() + dl->n : nullptr;
    g.cull = cmd.cull;
    g.keep = keep_tab ? S.keep_tab.get() : nullptr;
    f.gpars[f.lane] = par; cmd.par = par; cmd.lane = f.lane;
    GeomPass &gp = f.geom;
    gp.pred = cmd.pred;
    gp.set = si;
    gp.fan_cap = (uint32_t)fan_cap;
    gp.nblocks = nblocks;
    gp.seq = cmd.seq;
    gp.nitems = dl || it ? nmat : 1; gp.stride = m.ntris;
    // what the setup list about to be built was filtered by (frr_raster / frr_readback_setup check it), under which partition
    gp.part_rank = f.bound.rank; gp.part_world = f.bound.world; gp.part_blocked = f.bound.part_blocked;
    GeomRead rd;   // (from scratch: nothing of the previous pass stays)
    rd.filter = cmd.filter ? 1 : 0; rd.fy0 = cmd.fy0; rd.fy1 = cmd.fy1;
    rd.vs = vs; rd.ntris = nt;
    rd.mesh = m.dev; rd.mesh_gen = m.gen;
    rd.list = cmd.list; rd.list_gen = dl ? dl->gen : 0;
    rd.duni_hash = geom_uniform_digest(cmd.duni);
    rd.tex_epoch = c->tex_epoch; rd.cull = cmd.cull;
    rd.inst = it ? it->dev : nullptr; rd.inst_gen = it ? it->gen : 0; rd.ninst = it ? it->n : 0;
    rd.sync_epoch = (dl ? !dl->any_dev : m.own_dev && (!it || it->own || !it->n)) ? 0 : c->sync_epoch;   // (a host-uploaded mesh or table cannot change under the library)
    gp.read = rd;
    f.tris_in += nt; f.draws += 1;
    if (nt == 0) {
        hipLaunchKernelGGL(k_geom_empty, dim3(1), dim3(64), 0, gstream_of(c), g);
    } else {
        launch_geometry_vs(c, g, nblocks, vs, cmd.duni, um, dl ? dl->models.get() : it ? it->dev : nullptr, cmd.pv, cmd.keep, cmd.min_value);
        f.geom.scan_pending = true;
    }
    HIP_TRY(c, hipGetLastError());
    return FRR_OK;
}

// frr_query_pixels behind exec_raster's binning: k_visible_prep zeroes the caller's buffer and builds the item boundaries,
// k_query (frr_query.h) counts in the tile kernel's place.  No target is written, so the launches take the stream cmd_stream
// gives a command that writes none (exec_raster has ordered it behind the pass's geometry and binning).
int list_item_first(frr_ctx *c, const uint32_t **item_first);
template <bool ITEM, bool HIST> void launch_query_nw(hipStream_t ts, uint32_t grid, int nw, const RasterArgs &a, const QueryArgs &qa, int win_safe)
{
    if (nw == LIGHT_NW) hipLaunchKernelGGL((k_query<ITEM, HIST, LIGHT_NW>), dim3(grid), dim3(LIGHT_NW * 64), 0, ts, a, qa, win_safe);
    else if (nw == 4) hipLaunchKernelGGL((k_query<ITEM, HIST, 4>), dim3(grid), dim3(256), 0, ts, a, qa, win_safe);
    else if (nw == 6) hipLaunchKernelGGL((k_query<ITEM, HIST, 6>), dim3(grid), dim3(384), 0, ts, a, qa, win_safe);
    else if (nw == 8) hipLaunchKernelGGL((k_query<ITEM, HIST, 8>), dim3(grid), dim3(512), 0, ts, a, qa, win_safe);
    else hipLaunchKernelGGL((k_query<ITEM, HIST, 16>), dim3(grid), dim3(1024), 0, ts, a, qa, win_safe);
}
// What the two count commands (frr_visible_pixels, frr_query_pixels) share in front of their counting kernel: the arguments of
// k_visible_prep -- the window, the unit, the caller's buffer, the pass's id tables and, `bounds`: per item with something to
// count, the boundary table of the stream the command runs on -- and its launch (the zeros, the boundaries).  The items form
// of exec_shade takes the boundaries alone the same way.
int count_args(frr_ctx *c, const Cmd &cmd, hipStream_t ts, uint32_t ntris, bool bounds, const uint32_t *item_first, VisibleArgs *out)
{
    const FrameState &f = c->fs;
    const GeomSet &S = c->gset[f.geom.set];
    const int64_t wh = (int64_t)cmd.y1 - cmd.y0;
    VisibleArgs a;
    memset(&a, 0, sizeof a);
    a.x0 = cmd.x0; a.x1 = cmd.x1; a.y0 = cmd.y0; a.y1 = cmd.y1;
    a.unit = cmd.vis_unit;
    a.ntris = ntris;
    a.tinfo = S.tinfo; a.block_prefix = S.block_prefix;
    if (bounds) {
        DevBuf<uint32_t> &tab = c->vis_bounds[stream_slot(c, ts)];
        const int rc = ensure(c, tab, (size_t)f.geom.nitems + 1);
        if (rc != FRR_OK) return rc;
        a.nitems = (uint32_t)f.geom.nitems; a.item_first = item_first; a.stride = (uint32_t)f.geom.stride; a.bounds = tab;
    }
    a.gpar = f.gpar(); a.lane = f.lane;
    a.own = row_owner(f, (int)((wh + TILE - 1) / TILE));
    a.seq = cmd.seq; a.epoch = c->epoch; a.cnt = c->cnt;
    a.tri_id = f.bound.tri_id; a.out = cmd.vis_out; a.out_entries = cmd.vis_entries;
    *out = a;
    return FRR_OK;
}
void launch_count_prep(hipStream_t ts, const VisibleArgs &a)
{
    const uint64_t pn = std::max<uint64_t>(a.out_entries, (uint64_t)a.nitems + 1);
    hipLaunchKernelGGL(k_visible_prep, dim3((uint32_t)std::min<uint64_t>((pn + VIS_WG - 1) / VIS_WG, 2048)), dim3(VIS_WG), 0, ts, a);
}

int launch_query(frr_ctx *c, Cmd &cmd, const RasterArgs &a, uint32_t grid, const SpanShape sh, GeomSet &S, BinSet &B)
{
    FrameState &f = c->fs;
    int rc;
    const bool item = cmd.vis_unit == FRR_PER_ITEM;
    const uint32_t *item_first = nullptr;
    if (item && (rc = list_item_first(c, &item_first)) != FRR_OK) return rc;
    hipStream_t ts;
    if ((rc = cmd_stream(c, false, false, &ts)) != FRR_OK) return rc;
    VisibleArgs v;
    if ((rc = count_args(c, cmd, ts, (uint32_t)f.geom.read.ntris, item, item_first, &v)) != FRR_OK) return rc;
    {
        ProfScope p(c, KID_VISIBLE, ts);
        launch_count_prep(ts, v);
    }
    QueryArgs qa;
    qa.unit = cmd.vis_unit; qa.nitems = v.nitems; qa.bounds = v.bounds; qa.out = cmd.vis_out; qa.out_entries = cmd.vis_entries;
    qa.sweep_all = c->raster_sweep ? 1 : 0;
    const int win_safe = a.x0 >= -SPAN_SAFE && a.y0 >= -SPAN_SAFE && a.x1 <= SPAN_SAFE && a.y1 <= SPAN_SAFE;
    // per item the units that fit take the LDS histogram (option visible_lds_bins lowers the threshold: the test hook)
    const uint32_t cap = c->visible_lds_bins ? c->visible_lds_bins : VIS_LDS_BINS;
    const bool hist = item && std::min<uint64_t>(f.geom.nitems, cmd.vis_entries) <= cap;
    if (grid) {
        ProfScope p(c, KID_RASTER, ts);
        const int nw = c->raster_sweep ? 4 : sh.nw;
        if (item && hist) launch_query_nw<true, true>(ts, grid, nw, a, qa, win_safe);
        else if (item) launch_query_nw<true, false>(ts, grid, nw, a, qa, win_safe);
        else launch_query_nw<false, false>(ts, grid, nw, a, qa, win_safe);
    }
    HIP_TRY(c, hipGetLastError());
    return tile_launched(c, ts, S, B);
}

// Loop B (phong.rs:361-381): binning + tile kernel over the latest geometry pass, window (x0,x1) x (y0,y1)
int exec_raster(frr_ctx *c, Cmd &cmd)
{
    FrameState &f = c->fs;
    const int32_t x0 = cmd.x0, x1 = cmd.x1, y0 = cmd.y0, y1 = cmd.y1;
    const int ps_id = cmd.ps;
    const int64_t ww = (int64_t)x1 - x0, wh = (int64_t)y1 - y0;
    const UserModule *um = nullptr;
    if (ps_id >= FRR_SHADER_USER_BASE) { const int rcu = user_module(c, ps_id, &um); if (rcu != FRR_OK) return rcu; }
    bool fuse = false;
    if (f.clear.pending) {
        const bool full = x0 == 0 && y0 == 0 && x1 == (int32_t)c->W && y1 == (int32_t)c->H;
        if (full && !c->raster_sweep && !cmd.query) fuse = true; // the tile kernel performs the clear (a query writes no target: never)
        else { int rcs = settle_targets(c); if (rcs != FRR_OK) return rcs; }
    }
    GeomSet &S = c->gset[f.geom.set];
    RasterArgs a;
    a.fused_clear = fuse ? 1 : 0; a.clear_rgba = f.clear.rgba; a.clear_depth = f.clear.depth;
    a.x0 = x0; a.x1 = x1; a.y0 = y0; a.y1 = y1; a.win_w = (int)ww; a.win_h = (int)wh;
    a.cstride = (int)c->W; a.dstride = x1;
    a.tiles_x = (int)((ww + TILE - 1) / TILE); a.tiles_y = (int)((wh + TILE - 1) / TILE);
    a.tiles_x_magic = 0u; // set below once the grid is known (exact only for block indices and tile counts < 2^16)
    a.own = row_owner(f, a.tiles_y);
    a.recs = S.recs; a.vary = S.vary; a.pbox = S.pbox; a.bcount = S.bcount;
    a.tinfo = S.tinfo; a.fanbase = S.fanbase; a.fan_okey = S.fan_okey; a.block_prefix = S.block_prefix; a.ntris_draw = (uint32_t)f.geom.read.ntris;
    a.tile_counts = c->tile_counts; a.tile_offsets = c->tile_offsets; a.tile_cursor = c->tile_cursor;
    a.gpar = f.gpar(); a.lane = f.lane; a.bpar = 0; a.seq = cmd.seq; a.epoch = c->epoch; a.frame_no = f.frame_no; a.geom_seq = f.geom.seq;
    const uint32_t ntiles = (uint32_t)a.tiles_x * a.tiles_y;
    a.color = f.bound.color; a.depth = f.bound.depth; a.tri_id = f.bound.tri_id; a.cnt = c->cnt;
#ifdef FRR_DEBUG_COUNTERS
    if (!c->dbg_tiles && getenv("FRR_DEBUG_TILES")) (void)c->dbg_tiles.reset((size_t)c->max_tiles * 8);   // (empty if that fails)
    if (c->dbg_tiles) (void)hipMemsetAsync(c->dbg_tiles, 0, (size_t)c->max_tiles * 64, tstream_of(c));
    a.dbg_tiles = c->dbg_tiles;
#endif
    a.seg = nullptr; a.nseg = 0;
    a.tile_perm = nullptr; a.tile_cost = nullptr;
    const int owned_rows = a.own.blocked ? a.own.brow1 - a.own.brow0 : (a.tiles_y > f.bound.rank ? (a.tiles_y - f.bound.rank + f.bound.world - 1) / f.bound.world : 0);
    const uint32_t grid = (uint32_t)a.tiles_x * owned_rows;
    if (a.tiles_x >= 2 && a.tiles_x < 65536 && grid < 65536u) a.tiles_x_magic = (uint32_t)(0x100000000ull / (uint64_t)a.tiles_x + 1ull);
    const SpanShape sh = span_shape(c, grid, f.geom.read.ntris, ps_id);
    const bool segmented = grid <= BIN_LDS_MAX_TILES && !c->bin_atomics && !c->raster_sweep;
    const int q = segmented ? (f.bpar() ^ 1) : 0;   // (the CSR fallback has one set of tile tables: it uses workspace 0 and overlaps nothing)
    const int bi = !segmented ? 0 : f.geom.on_g ? (f.bset ^ 1) : (frames_alternate(c) ? f.bound.tset : 0);
    BinSet &B = c->bset[bi];
    int rc;
    if (!B.bins) {
        size_t want = std::max<size_t>((size_t)f.geom.read.ntris * 8 + 4 * (size_t)c->max_tiles, (size_t)1 << 22);
        if (c->bin_cap_init) want = c->bin_cap_init;      // option bin_capacity (tests of the replay)
        want = std::max(want, c->bset[bi ^ 1].bins.cap());   // (what the other workspace has grown to)
        if ((rc = ensure(c, B.bins, want)) != FRR_OK) return rc;
        if ((rc = ensure(c, B.bins2, want)) != FRR_OK) return rc;
    }
    a.bins2 = B.bins2;
    a.bins = B.bins; a.bin_cap = (uint32_t)std::min<size_t>(B.bins.cap(), 0xFFFFFFFFu);
    hipStream_t gs = gstream_of(c);
    if (segmented) {
        const uint32_t ltiles = std::max<uint32_t>(grid, 1u);   // the binning numbers the rank's OWN tiles only (local_tile_row)
        // segmented LDS multi-split (one launch, no per-entry global atomics): G chunk workgroups, ~3K triangles each
        // (small meshes: one triangle per thread, so that the launch is not three workgroups doing all the work)
        uint32_t G = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((f.geom.read.ntris + BIN_WG - 1) / BIN_WG, 1), BIN_MAX_G);
        if (c->bin_g > 0) G = (uint32_t)std::min(c->bin_g, BIN_MAX_G);
        G = std::min<uint32_t>(G, sh.nw == 3 ? 256u : (uint32_t)sh.nw * 64u); // the tile kernel reads one segment per thread (three waves: wave 0 reads a second one)
        // Option tile_order 1: the tile kernel records each tile's records in tile_cost; a later pass over the same grid on
        // this set orders its blocks heaviest first by them (build_tile_perm).  Measured no faster than the fixed order
        // (DESIGN.md section 5), so off by default: then nothing is recorded and nothing built.
        bool fresh_cost;
        if ((rc = ensure(c, B.tile_cost, ltiles, &fresh_cost)) != FRR_OK) return rc;
        if ((rc = ensure(c, B.tile_perm, ltiles)) != FRR_OK) return rc;
        if (fresh_cost) {   // new memory: no costs recorded yet (and defined ones until a tile kernel writes them)
            B.cost_known = false;
            HIP_TRY(c, hipMemsetAsync(B.tile_cost, 0, (size_t)ltiles * sizeof(uint32_t), gs));
        }
        const TileOrderKey okey = {grid, a.tiles_x, x0, x1, y0, y1, f.bound.rank, f.bound.world, a.own.blocked, sh.nw};
        const bool ordered = tile_order_built(c->tile_order, c->in_replay, okey, B.cost_known, B.cost_key);
        const bool record = c->tile_order == TILE_ORDER_HEAVY_FIRST;
        a.tile_cost = record ? B.tile_cost : nullptr;
        a.tile_perm = ordered ? B.tile_perm : nullptr;
        const uint32_t perm_seed = c->tile_order == TILE_ORDER_RANDOM ? (uint32_t)fnv1a(&cmd.seq, sizeof cmd.seq) | 1u : 0u;
        // (+ one workgroup that scans the geometry kernel's block sums, unless an earlier launch has, and builds the order;
        // a binning workgroup fills a CU's LDS, so the launch stays within 256 workgroups: a 257th would wait for a whole
        // one to finish)
        const int do_scan = f.geom.scan_pending ? 1 : 0;
        const uint32_t extra = (do_scan || ordered) ? 1u : 0u;
        if (extra && G > 255u) G = 255u;
        if ((rc = ensure(c, B.bin_matrix, (size_t)BIN_MAX_G * ((size_t)c->max_tiles + 1))) != FRR_OK) return rc;
        // dynamic LDS: tile counters + as many staged 16-B records as fit (a chunk emits ~1.8 records per triangle)
        constexpr size_t kLdsBudget = 160 * 1024 - 1024; // the kernel's static LDS is < 1 KB
        const size_t hist_bytes = (((size_t)ltiles + 3) & ~(size_t)3) * sizeof(uint32_t);
        const uint32_t stage_cap = (uint32_t)std::min<size_t>((kLdsBudget - hist_bytes) / 16, 9216);
        const size_t lds = hist_bytes + (size_t)stage_cap * 16;
        if (!c->lds_attr_set) {
            HIP_TRY(c, hipFuncSetAttribute((const void *)k_bin_seg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
            c->lds_attr_set = true;
        }
        a.seg = B.bin_matrix; a.nseg = G; a.bpar = q;
        // near-first copies (bins2): a fixed slot per tile, 8x the mean tile load, + an overflow arena of bin_cap records
        uint64_t SL = std::max<uint64_t>(256, (f.geom.read.ntris * 16 + ntiles - 1) / ntiles);   // (per-tile load of the whole window: ownership does not change it)
        SL = std::min<uint64_t>(SL, ((uint64_t)1 << 30) / ltiles);
        if (c->ent_slot_override) SL = c->ent_slot_override;
        a.ent_slot = (uint32_t)SL;
        a.bin_cap = (uint32_t)std::min<size_t>(B.bins.cap(), 0xBFFFFFFFu);
        if ((rc = ensure(c, B.bins2, (size_t)ltiles * SL + a.bin_cap)) != FRR_OK) return rc;
        a.bins2 = B.bins2;
        if ((rc = gstream_wait_readers(c, B.reader)) != FRR_OK) return rc;   // the tile kernel that last read this workspace
        {
            ProfScope p(c, KID_BIN_SEG, gs);
            hipLaunchKernelGGL(k_bin_seg, dim3(G + extra), dim3(BIN_WG), lds, gs, a, ltiles, B.bin_matrix, stage_cap,
                               f.geom.fan_cap, S.block_sums, S.block_prefix, f.geom.nblocks, do_scan | (cmd.query ? 2 : 0), perm_seed);
        }
        // The tile kernel launched below writes every tile's cost -- unless the pass is cancelled (a list overflowed): then
        // the costs stay what an earlier pass (or the zeroing above) left, and the replay of the pass writes them.  Any values
        // give a permutation (build_tile_perm); only how well it orders depends on them.
        if (!cmd.query) { B.cost_known = record; B.cost_key = okey; }   // (a query's kernel records no costs: what the set holds stays what it was)
        if (ordered) ++c->ordered_passes;
        f.geom.scan_pending = false;
        f.bpars[f.lane] = q; f.bset = bi;
    } else {
        // fallback for frames with more tiles than fit LDS counters: global atomics (one set of tile tables: after every
        // tile kernel so far)
        for (GeomSet &G2 : c->gset) if ((rc = gstream_wait_readers(c, G2.reader)) != FRR_OK) return rc;
        for (BinSet &B2 : c->bset) if ((rc = gstream_wait_readers(c, B2.reader)) != FRR_OK) return rc;
        if ((rc = scan_now(c)) != FRR_OK) return rc;
        const uint32_t bin_grid = (uint32_t)std::min<uint64_t>((f.geom.read.ntris + f.geom.fan_cap + 255) / 256, 2048);
        { ProfScope p(c, KID_BIN_COUNT, gs); hipLaunchKernelGGL(k_bin<false>, dim3(bin_grid), dim3(256), 0, gs, a, f.geom.fan_cap); }
        { ProfScope p(c, KID_TILE_SCAN, gs); if (cmd.query) hipLaunchKernelGGL(k_tile_scan_uncounted, dim3(1), dim3(1024), 0, gs, a, ntiles); else hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(1024), 0, gs, a, ntiles); }
        { ProfScope p(c, KID_BIN_FILL, gs); hipLaunchKernelGGL(k_bin<true>, dim3(bin_grid), dim3(256), 0, gs, a, f.geom.fan_cap); }
    }
    cmd.par = q; cmd.set = bi; cmd.lane = f.lane;
    HIP_TRY(c, hipGetLastError());
    if (!c->in_replay) {
        // does this pass's need of the work lists fit for sure?  (exec_cmd waits for the event if not: frr_ctx::proven)
        const DrawSig sig = draw_sig(f.geom.read, x0, x1, y0, y1, f.bound.rank, f.bound.world, f.bound.part_blocked, f.geom.set, bi, c->join_epoch);
        if (!c->proven.known(sig, f.geom.pred)) {
            HIP_TRY(c, hipEventRecord(c->ev_verify, gs));
            c->verify_pending = true;
            c->verify_pred = f.geom.pred;
            c->verify_sig = sig;
        }
    }
    if ((rc = tstream_wait_gstream(c)) != FRR_OK) return rc;   // the tile kernel runs on the targets' stream, after the binning
    if (cmd.query) return launch_query(c, cmd, a, grid, sh, S, B);
    // frr_frame_wait: the targets' next writer follows what those streams held (a replay re-issues an earlier write: it
    // waits too, but leaves the waits to the write they were asked for)
    hipStream_t ts;
    if ((rc = target_write(c, !c->in_replay, &ts)) != FRR_OK) return rc;
    // x0 < 0: the depth stride x1 is smaller than the window's width and pixels of neighbouring rows share depth entries,
    // which only a resolve per ENTRY reproduces (k_raster_entries).  On a partitioned ctx the pixels of an entry belong to
    // different ranks, each with a depth buffer of its own: there the tile kernels run as for any window.
    const bool shared_entries = ww > (int64_t)x1 && f.bound.world <= 1;
    // the span algebra needs every coordinate it touches within +-SPAN_SAFE (no i32 wrap)
    const int win_safe = a.x0 >= -SPAN_SAFE && a.y0 >= -SPAN_SAFE && a.x1 <= SPAN_SAFE && a.y1 <= SPAN_SAFE;
    if (grid && shared_entries) {
        ProfScope p(c, KID_RASTER, ts);
        const unsigned eg = (unsigned)((((wh - 1) * (int64_t)x1 + ww) + 255) / 256);
        if (um) {
            RasterArgs ra = a; DevUniforms d = cmd.duni;
            void *args[] = {&ra, &d};
            (void)hipModuleLaunchKernel(um->entries, eg, 1, 1, 256, 1, 1, 0, ts, args, nullptr);
        } else {
            switch (ps_id) {
            case FRR_PS_DEPTH: hipLaunchKernelGGL((k_raster_entries<0, FRR_PS_DEPTH>), dim3(eg), dim3(256), 0, ts, a, cmd.duni); break;
            case FRR_PS_FLAT: hipLaunchKernelGGL((k_raster_entries<0, FRR_PS_FLAT>), dim3(eg), dim3(256), 0, ts, a, cmd.duni); break;
            case FRR_PS_COLOR: hipLaunchKernelGGL((k_raster_entries<3, FRR_PS_COLOR>), dim3(eg), dim3(256), 0, ts, a, cmd.duni); break;
            case FRR_PS_PHONG: hipLaunchKernelGGL((k_raster_entries<8, FRR_PS_PHONG>), dim3(eg), dim3(256), 0, ts, a, cmd.duni); break;
            case FRR_PS_BLINN: hipLaunchKernelGGL((k_raster_entries<8, FRR_PS_BLINN>), dim3(eg), dim3(256), 0, ts, a, cmd.duni); break;
            }
        }
    } else if (grid && um) {
        ProfScope p(c, KID_RASTER, ts);
        int shi = 4;
        for (int k = 0; k < 6; ++k) if (kSpanShapes[k][0] == sh.nw && kSpanShapes[k][1] == sh.occ) shi = k;
        RasterArgs ra = a; DevUniforms d = cmd.duni; int ws = win_safe;
        void *args[] = {&ra, &d, &ws};
        if (c->raster_sweep) (void)hipModuleLaunchKernel(um->sweep, grid, 1, 1, 256, 1, 1, 0, ts, args, nullptr);   // k_raster(RasterArgs, DevUniforms)
        else (void)hipModuleLaunchKernel(um->span[cmd.count_frags ? 1 : 0][shi], grid, 1, 1, (unsigned)kSpanShapes[shi][0] * 64u, 1, 1, 0, ts, args, nullptr);
    } else if (grid) {
        switch (ps_id) {
        case FRR_PS_DEPTH: launch_raster<0, FRR_PS_DEPTH>(c, ts, a, grid, sh, cmd.duni, cmd.count_frags, win_safe); break;
        case FRR_PS_FLAT: launch_raster<0, FRR_PS_FLAT>(c, ts, a, grid, sh, cmd.duni, cmd.count_frags, win_safe); break;
        case FRR_PS_COLOR: launch_raster<3, FRR_PS_COLOR>(c, ts, a, grid, sh, cmd.duni, cmd.count_frags, win_safe); break;
        case FRR_PS_PHONG: launch_raster<8, FRR_PS_PHONG>(c, ts, a, grid, sh, cmd.duni, cmd.count_frags, win_safe); break;
        case FRR_PS_BLINN: launch_raster<8, FRR_PS_BLINN>(c, ts, a, grid, sh, cmd.duni, cmd.count_frags, win_safe); break;
        }
    }
    HIP_TRY(c, hipGetLastError());
    if ((rc = tile_launched(c, ts, S, B)) != FRR_OK) return rc;
    if (fuse) {
        f.clear.pending = false;
        // the tile rows of other ranks missed this clear: owed to the ctx's own targets (frr_readback shows the
        // whole image); caller-bound targets of a partitioned ctx only ever have their owned rows defined
        f.clear.unowned_debt = f.bound.world > 1 && own_targets(c);
        f.clear.debt_tiles_y = a.tiles_y;
    }
    return FRR_OK;
}

// FrameBuffer::draw_line (renderer.rs:540-588) for every segment of a list, in list order, or for the edges of the latest
// geometry pass's triangles: colour only.  It writes a target; the wireframe also reads the pass.
int exec_lines(frr_ctx *c, Cmd &cmd)
{
    FrameState &f = c->fs;
    const bool wire = cmd.lines < 0;
    int rc;
    if ((rc = cmd_settle(c, wire)) != FRR_OK) return rc;
    LinesArgs a;
    memset(&a, 0, sizeof a);
    uint32_t batches;
    if (wire) {
        const GeomSet &S = c->gset[f.geom.set];
        a.recs = S.recs; a.tinfo = S.tinfo; a.fan_cap = f.geom.fan_cap; a.wire_rgba = cmd.wire_rgba;
        a.gpar = f.gpar(); a.lane = f.lane;
        batches = (uint32_t)((3ull * (f.geom.read.ntris + f.geom.fan_cap) + 63) / 64);
    } else {
        const Lines &L = c->lines[cmd.lines];
        a.xyxy = L.xyxy; a.rgba = L.rgba; a.nlines = (uint32_t)L.n;
        batches = (uint32_t)((L.n + 63) / 64);
    }
    hipStream_t ts;
    if ((rc = cmd_stream(c, wire, true, &ts)) != FRR_OK) return rc;
    // (a device-bound list needs no join of `ts` with the caller's stream: frr_lines_bind_device has waited on the host for
    // that stream, behind whatever wrote the list)
    DevBuf<uint32_t> &owner = c->line_owner[stream_slot(c, ts)];
    if (!owner) {
        const size_t npx = (size_t)c->W * c->H;
        if (owner.reset(npx) != hipSuccess) return nomem(c, "owner plane");
        const hipError_t e = hipMemsetAsync(owner, 0, npx * sizeof(uint32_t), ts);
        if (e != hipSuccess) { (void)owner.release(); return fail(c, FRR_ERR_HIP, std::string("hipMemsetAsync owner plane: ") + hipGetErrorString(e)); }
    }
    a.W = c->W; a.H = c->H;
    a.own = row_owner(f, (int)((c->H + TILE - 1) / TILE));
    a.chunk = c->lines_chunk ? c->lines_chunk : LINES_CHUNK;
    a.seq = cmd.seq; a.epoch = c->epoch; a.cnt = c->cnt;
    a.owner = owner; a.color = (uint32_t *)f.bound.color;
    const dim3 grid(std::max<uint32_t>(std::min<uint32_t>(batches, 16384u), 1u)), block(64);
    {
        ProfScope p(c, KID_LINES_MARK, ts);
        if (wire) hipLaunchKernelGGL(k_lines_mark<true>, grid, block, 0, ts, a);
        else hipLaunchKernelGGL(k_lines_mark<false>, grid, block, 0, ts, a);
    }
    {
        ProfScope p(c, KID_LINES_PAINT, ts);
        if (wire) hipLaunchKernelGGL(k_lines_paint<true>, grid, block, 0, ts, a);
        else hipLaunchKernelGGL(k_lines_paint<false>, grid, block, 0, ts, a);
    }
    HIP_TRY(c, hipGetLastError());
    cmd_done(c, cmd, wire, ts);
    return FRR_OK;
}

// frr_resolve_varyings: the interpolated varyings (renderer.rs:368-378) of every pixel of the window that a triangle of the
// latest geometry pass owns, into the caller's buffer (frr_varyings.h).  It reads the pass and writes no target.
int exec_vary(frr_ctx *c, Cmd &cmd)
{
    FrameState &f = c->fs;
    int rc;
    if ((rc = cmd_settle(c, true)) != FRR_OK) return rc;
    GeomSet &S = c->gset[f.geom.set];
    const int par = f.gpar();
    bool fresh_table;
    if ((rc = ensure(c, S.vslot[par], S.recs.cap(), &fresh_table)) != FRR_OK) return rc;
    if (fresh_table) S.vslot_seq[par] = 0;   // new memory: no table
    hipStream_t ts;
    if ((rc = cmd_stream(c, true, false, &ts)) != FRR_OK) return rc;
    if (S.vslot_stream[par] && S.vslot_stream[par] != ts) {   // the table's previous resolve ran on another stream: after it
        HIP_TRY(c, hipEventRecord(c->ev_join, S.vslot_stream[par]));
        HIP_TRY(c, hipStreamWaitEvent(ts, c->ev_join, 0));
    }
    S.vslot_stream[par] = ts;
    const int64_t ww = (int64_t)cmd.x1 - cmd.x0, wh = (int64_t)cmd.y1 - cmd.y0;
    VaryArgs a;
    memset(&a, 0, sizeof a);
    a.x0 = cmd.x0; a.x1 = cmd.x1; a.y0 = cmd.y0; a.y1 = cmd.y1;
    a.K = frr_vs_num_varyings(f.geom.read.vs);
    a.recs = S.recs; a.vary = S.vary; a.tinfo = S.tinfo; a.fan_okey = S.fan_okey; a.block_prefix = S.block_prefix;
    a.table = S.vslot[par];
    a.setup_cap = (uint32_t)std::min<size_t>(std::min(S.recs.cap(), S.vslot[par].cap()), 0xFFFFFFFFu); a.fan_cap = f.geom.fan_cap;
    a.ntris = (uint32_t)f.geom.read.ntris;
    a.gpar = par; a.lane = f.lane;
    a.own = row_owner(f, (int)((wh + TILE - 1) / TILE));
    a.seq = cmd.seq; a.epoch = c->epoch; a.cnt = c->cnt;
    a.tri_id = f.bound.tri_id; a.out = cmd.vary_out;
    if (S.vslot_seq[par] != f.geom.seq || S.vslot_epoch[par] != c->epoch) {   // (else: an earlier resolve of this pass built the table)
        const uint32_t sgrid = (uint32_t)std::min<uint64_t>((f.geom.read.ntris + f.geom.fan_cap + VARY_WG - 1) / VARY_WG, 4096);
        hipLaunchKernelGGL(k_vary_slots, dim3(std::max<uint32_t>(sgrid, 1u)), dim3(VARY_WG), 0, ts, a);
        S.vslot_seq[par] = f.geom.seq; S.vslot_epoch[par] = c->epoch;
    }
    const dim3 grid((unsigned)((ww + VARY_WG - 1) / VARY_WG), (unsigned)wh), block(VARY_WG);
    // 16-byte stores where every entry's address allows them: K a multiple of 4 and an aligned buffer
    const bool vec = (a.K & 3) == 0 && (((uintptr_t)a.out | (uintptr_t)a.vary) & 15u) == 0u;
    if (a.K == 3) hipLaunchKernelGGL((k_vary_resolve<3, false>), grid, block, 0, ts, a);
    else if (a.K == 8 && vec) hipLaunchKernelGGL((k_vary_resolve<8, true>), grid, block, 0, ts, a);
    else if (a.K == 8) hipLaunchKernelGGL((k_vary_resolve<8, false>), grid, block, 0, ts, a);
    else if (vec) hipLaunchKernelGGL((k_vary_resolve<0, true>), grid, block, 0, ts, a);   // user shaders: K at run time
    else hipLaunchKernelGGL((k_vary_resolve<0, false>), grid, block, 0, ts, a);
    HIP_TRY(c, hipGetLastError());
    cmd_done(c, cmd, true, ts);
    return FRR_OK;
}

// *item_first: where the latest geometry pass, a list pass, keeps the first triangle of every item (GeomArgs::item_first); else null
int list_item_first(frr_ctx *c, const uint32_t **item_first)
{
    const GeomRead &rd = c->fs.geom.read;
    *item_first = nullptr;
    if (rd.list < 0) return FRR_OK;
    if (!slot_ok(c->lists, rd.list) || c->lists[rd.list].gen != rd.list_gen) return fail(c, FRR_ERR_INVALID, "the draw list of the latest geometry pass was freed");
    *item_first = c->lists[rd.list].first;
    return FRR_OK;
}

// frr_visible_pixels: the triangle-id target of a window as counts per item of the latest geometry pass, or per triangle of
// the frame (frr_visible.h).  It reads the pass and writes no target; behind a failed command not even the zeros are written.
int exec_visible(frr_ctx *c, Cmd &cmd)
{
    FrameState &f = c->fs;
    int rc;
    if ((rc = cmd_settle(c, true)) != FRR_OK) return rc;
    const bool item = cmd.vis_unit == FRR_PER_ITEM;
    const bool cleared = f.draws == 0;   // frr_clear since the pass: the id target holds nothing of it, and its tables are gone
    const uint32_t *item_first = nullptr;
    if (item && !cleared && !cmd.query && (rc = list_item_first(c, &item_first)) != FRR_OK) return rc;
    hipStream_t ts;
    if ((rc = cmd_stream(c, true, false, &ts)) != FRR_OK) return rc;
    // the units the histogram can meet: decides the path, and whether there is anything to count at all (a frr_query_pixels
    // with nothing to rasterize is this command with nothing to count: the zeros alone)
    const uint64_t bound = cleared || cmd.query ? 0 : item ? std::min<uint64_t>(f.geom.nitems, cmd.vis_entries) : cmd.vis_entries;
    const int64_t ww = (int64_t)cmd.x1 - cmd.x0, wh = (int64_t)cmd.y1 - cmd.y0;
    VisibleArgs a;
    if ((rc = count_args(c, cmd, ts, cleared ? 0u : (uint32_t)f.geom.read.ntris, item && bound > 0, item_first, &a)) != FRR_OK) return rc;
    const uint32_t cap = c->visible_lds_bins ? c->visible_lds_bins : VIS_LDS_BINS;
    const bool lds = bound <= cap;
    // rows per workgroup: a span is a chain of dependent loads, so what counts is waves in flight -- as many workgroups as
    // the window has rows, up to 2,048 -- but no fewer than 16 spans (four per wave) for a workgroup's set-up and flush
    const uint64_t spr = ((uint64_t)ww + VIS_SPAN - 1) / VIS_SPAN;
    a.rows = (uint32_t)std::max<uint64_t>(std::min<uint64_t>(std::max<uint64_t>((16 + spr - 1) / spr, (uint64_t)(wh + 2047) / 2048), (uint64_t)wh), 1);
    {
        ProfScope p(c, KID_VISIBLE, ts);
        launch_count_prep(ts, a);
        if (bound > 0) {
            const dim3 grid((uint32_t)((wh + a.rows - 1) / a.rows)), block(VIS_WG);
            const bool blds = item && a.nitems <= VIS_LDS_BINS;   // the boundaries fit LDS too
            if (item && lds && blds) hipLaunchKernelGGL((k_visible<true, true, true>), grid, block, 0, ts, a);
            else if (item && lds) hipLaunchKernelGGL((k_visible<true, true, false>), grid, block, 0, ts, a);
            else if (item && blds) hipLaunchKernelGGL((k_visible<true, false, true>), grid, block, 0, ts, a);
            else if (item) hipLaunchKernelGGL((k_visible<true, false, false>), grid, block, 0, ts, a);
            else if (lds) hipLaunchKernelGGL((k_visible<false, true, false>), grid, block, 0, ts, a);
            else hipLaunchKernelGGL((k_visible<false, false, false>), grid, block, 0, ts, a);
        }
    }
    HIP_TRY(c, hipGetLastError());
    cmd_done(c, cmd, true, ts);
    return FRR_OK;
}

// frr_shade_varyings, frr_shade_items: a pixel shader over a buffer of varyings into the colour target (frr_shade.h), under
// the uniforms of the call (k_shade_vary, over a range of triangle ids) or under the material of each pixel's item
// (k_shade_items).  Both write a target; the items form also reads the pass -- it finds a pixel's item in the boundaries a
// per-item count builds, built here the same way, into the same per-stream table -- and a replay reads the material table
// as it is then.
ShadeArgs shade_args(const frr_ctx *c, const Cmd &cmd)
{
    const FrameState &f = c->fs;
    const int64_t wh = (int64_t)cmd.y1 - cmd.y0;
    ShadeArgs a;
    memset(&a, 0, sizeof a);
    a.x0 = cmd.x0; a.x1 = cmd.x1; a.y0 = cmd.y0; a.y1 = cmd.y1;
    a.cstride = (int32_t)c->W;
    a.own = row_owner(f, (int)((wh + TILE - 1) / TILE));
    a.id_first = cmd.id_first; a.id_count = cmd.id_count;   // (a SHADE_ITEMS command has none: zeros)
    a.seq = cmd.seq; a.epoch = c->epoch; a.cnt = c->cnt;
    a.tri_id = f.bound.tri_id; a.in = cmd.shade_in; a.in_entries = cmd.shade_entries;
    a.color = (uint32_t *)f.bound.color;
    return a;
}
// items: k_shade_items over `a`, else k_shade_vary over a.s
template <int K, int PS> void launch_shade(hipStream_t ts, dim3 grid, bool items, const ShadeItemsArgs &a, const DevUniforms &du, bool vec)
{
    auto go = [&](auto vec_tag) {
        constexpr bool VEC = decltype(vec_tag)::value;
        if (items) hipLaunchKernelGGL((k_shade_items<K, PS, VEC>), grid, dim3(SHADE_WG), 0, ts, a, du);
        else hipLaunchKernelGGL((k_shade_vary<K, PS, VEC>), grid, dim3(SHADE_WG), 0, ts, a.s, du);
    };
    if constexpr (K > 0 && K % 4 == 0) { if (vec) { go(std::true_type{}); return; } }
    go(std::false_type{});
}
int exec_shade(frr_ctx *c, Cmd &cmd)
{
    FrameState &f = c->fs;
    const bool items = cmd.kind == Cmd::SHADE_ITEMS;
    int rc;
    const UserModule *um = nullptr;
    if (cmd.ps >= FRR_SHADER_USER_BASE && (rc = user_module(c, cmd.ps, &um)) != FRR_OK) return rc;
    if ((rc = cmd_settle(c, items)) != FRR_OK) return rc;
    const uint32_t *item_first = nullptr;
    if (items && (rc = list_item_first(c, &item_first)) != FRR_OK) return rc;
    hipStream_t ts;
    if ((rc = cmd_stream(c, items, true, &ts)) != FRR_OK) return rc;
    ShadeItemsArgs a;
    memset(&a, 0, sizeof a);
    a.s = shade_args(c, cmd);
    if (items) {
        VisibleArgs v;   // the boundaries, as a per-item count builds them: no counts, so nothing to zero
        if ((rc = count_args(c, cmd, ts, (uint32_t)f.geom.read.ntris, true, item_first, &v)) != FRR_OK) return rc;
        v.unit = FRR_PER_ITEM; v.out = nullptr; v.out_entries = 0;
        a.bounds = v.bounds; a.nitems = v.nitems; a.mats = cmd.mats; a.zero_tex = c->zero_texel;
        launch_count_prep(ts, v);
    }
    const int64_t ww = (int64_t)cmd.x1 - cmd.x0, wh = (int64_t)cmd.y1 - cmd.y0;
    const dim3 grid((unsigned)((ww + SHADE_WG - 1) / SHADE_WG), (unsigned)wh);
    // 16-byte loads where every entry's address allows them: K a multiple of 4 and an aligned buffer
    const bool vec = cmd.shade_K > 0 && (cmd.shade_K & 3) == 0 && ((uintptr_t)cmd.shade_in & 15u) == 0u;
    if (um) {
        DevUniforms d = cmd.duni;
        void *args[] = {items ? (void *)&a : (void *)&a.s, &d};
        (void)hipModuleLaunchKernel((items ? um->shade_items : um->shade)[vec ? 1 : 0], grid.x, grid.y, 1, SHADE_WG, 1, 1, 0, ts, args, nullptr);
    } else {
        switch (cmd.ps) {
        case FRR_PS_FLAT: launch_shade<0, FRR_PS_FLAT>(ts, grid, items, a, cmd.duni, false); break;   // (reads no varying, whatever K the buffer has)
        case FRR_PS_COLOR: launch_shade<3, FRR_PS_COLOR>(ts, grid, items, a, cmd.duni, false); break;
        case FRR_PS_PHONG: launch_shade<8, FRR_PS_PHONG>(ts, grid, items, a, cmd.duni, vec); break;
        case FRR_PS_BLINN: launch_shade<8, FRR_PS_BLINN>(ts, grid, items, a, cmd.duni, vec); break;
        }
    }
    HIP_TRY(c, hipGetLastError());
    cmd_done(c, cmd, items, ts);
    return FRR_OK;
}

// frr_query_boxes: the pyramid of the window's depth (k_box_base, k_box_top), then the test of every item of the list against
// it (k_box_test; frr_boxes.h).  It reads no pass and writes no target.  The levels: the first from BOX_LEVEL_MIN at which
// four cells span the window in both directions is the last.  Every extent grows with the window, so the layout of the
// whole viewport bounds the cells of any window: the buffer is allocated at that size on first use and never grown.
BoxPyramid box_pyramid_layout(int64_t ww, int64_t wh, size_t *cells)
{
    BoxPyramid p;
    memset(&p, 0, sizeof p);
    const uint32_t tx = (uint32_t)((ww + TILE - 1) / TILE), ty = (uint32_t)((wh + TILE - 1) / TILE);
    int top = BOX_LEVEL_MIN;
    while (((ww - 1) >> top) > 3 || ((wh - 1) >> top) > 3) ++top;
    p.top = top;
    size_t at = 0;
    for (int s = BOX_LEVEL_MIN; s <= std::max(top, (int)BOX_LEVEL_TILE); ++s) {   // (the base pass always writes its four levels)
        if (s <= BOX_LEVEL_TILE) { p.lw[s] = tx << (BOX_LEVEL_TILE - s); p.lh[s] = ty << (BOX_LEVEL_TILE - s); }
        else {
            const int k = s - BOX_LEVEL_TILE;
            p.lw[s] = (tx + (1u << k) - 1u) >> k; p.lh[s] = (ty + (1u << k) - 1u) >> k;
            p.top_cells += p.lw[s] * p.lh[s];
        }
        p.off[s] = (uint32_t)at;
        at += (size_t)p.lw[s] * p.lh[s];
    }
    *cells = at;
    return p;
}
int exec_boxes(frr_ctx *c, Cmd &cmd)
{
    FrameState &f = c->fs;
    int rc;
    if ((rc = cmd_settle(c, false)) != FRR_OK) return rc;
    const DrawList &dl = c->lists[cmd.list];   // (checked by the call; a list cannot go, nor its table change, while the command is logged)
    hipStream_t ts;
    if ((rc = cmd_stream(c, false, false, &ts)) != FRR_OK) return rc;
    const int64_t ww = (int64_t)cmd.x1 - cmd.x0, wh = (int64_t)cmd.y1 - cmd.y0;
    BoxArgs a;
    memset(&a, 0, sizeof a);
    size_t cells, most;
    a.pyr = box_pyramid_layout(ww, wh, &cells);
    (void)box_pyramid_layout((int64_t)c->W, (int64_t)c->H, &most);
    DevBuf<uint32_t> &pyr = c->box_pyr[stream_slot(c, ts)];
    if ((rc = ensure(c, pyr, std::max(cells, most))) != FRR_OK) return rc;   // (new memory on the slot's first use only: no drain, no host wait)
    a.pyr.cells = pyr;
    a.w = BoxWindow{c->W, c->H, cmd.x0, cmd.x1, cmd.y0, cmd.y1};
    a.tiles_x = (int32_t)((ww + TILE - 1) / TILE); a.tiles_y = (int32_t)((wh + TILE - 1) / TILE);
    a.own = row_owner(f, a.tiles_y);
    for (int t = 0; t < a.tiles_y; ++t) {
        if (owns_tile_row(t, a.own)) a.window_owned_rows += (uint32_t)std::min<int64_t>(TILE, wh - (int64_t)t * TILE);
    }
    a.depth = f.bound.depth; a.depth_vec = ((uintptr_t)f.bound.depth & 15u) == 0u ? 1 : 0;
    memcpy(a.pv.m, cmd.pv, sizeof a.pv.m);
    a.models = dl.models; a.lo_hi = dl.box_lo_hi; a.flags = dl.box_flags; a.nitems = (uint32_t)dl.n;
    a.out = cmd.vis_out; a.out_entries = cmd.vis_entries;
    a.seq = cmd.seq; a.epoch = c->epoch; a.cnt = c->cnt;
    {
        ProfScope p(c, KID_BOXES, ts);
        if (dl.n) {
            hipLaunchKernelGGL(k_box_base, dim3((uint32_t)(a.tiles_x * a.tiles_y)), dim3(256), 0, ts, a);
            if (a.pyr.top_cells) hipLaunchKernelGGL(k_box_top, dim3((a.pyr.top_cells + 3u) / 4u), dim3(256), 0, ts, a);
        }
        const uint64_t units = std::max<uint64_t>(dl.n, cmd.vis_entries);
        hipLaunchKernelGGL(k_box_test, dim3((uint32_t)std::min<uint64_t>((units + 15) / 16, 4096)), dim3(256), 0, ts, a);
    }
    HIP_TRY(c, hipGetLastError());
    cmd_done(c, cmd, false, ts);
    return FRR_OK;
}

int finish(frr_ctx *c);

// run a command and remember it (finish() replays the commands from a failed one onwards)
int exec_cmd(frr_ctx *c, Cmd cmd)
{
    // The previous pass's n_emit feeds a geometry pass's tri_base.  If no binning launch has scanned that pass's block sums
    // (it was never rastered), they are scanned here: before exec_geometry sizes the tables -- where both passes use one
    // set, a pass with more blocks reallocates block_sums, and writes its own sums there -- and before the snapshot a replay
    // of this command starts from, so that a replay does not scan again what this pass has overwritten by then.
    if (cmd.kind == Cmd::GEOM) { const int rs = scan_now(c); if (rs != FRR_OK) return rs; }
    cmd.pre = c->fs;
    cmd.seq = c->next_seq++;
    c->verify_pending = false;
    int rc = FRR_OK;
    switch (cmd.kind) {
    case Cmd::GEOM: rc = exec_geometry(c, cmd); break;
    case Cmd::RASTER: rc = exec_raster(c, cmd); break;
    case Cmd::LINES: rc = exec_lines(c, cmd); break;
    case Cmd::VARY: rc = exec_vary(c, cmd); break;
    case Cmd::VISIBLE: rc = exec_visible(c, cmd); break;
    case Cmd::SHADE: case Cmd::SHADE_ITEMS: rc = exec_shade(c, cmd); break;
    case Cmd::BOXES: rc = exec_boxes(c, cmd); break;
    }
    if (rc != FRR_OK) { c->fs = cmd.pre; c->verify_pending = false; return rc; }
    c->log.push_back(cmd);
    if (c->verify_pending) {
        // An unproven raster pass: wait for its binning launch (the tile kernel behind it is not waited for: it cancels itself
        // if the pass or its geometry found a list too small), then look at the word failed commands write to host memory.
        c->verify_pending = false;
        const DrawSig sig = c->verify_sig;
        bool failed = true;   // (no host-visible word: a full synchronisation point decides)
        if (c->host_bad) {
            HIP_TRY(c, hipEventSynchronize(c->ev_verify));
            failed = *(volatile uint32_t *)c->host_bad != c->seen_bad;
        }
        if (failed) { const int rf = finish(c); if (rf != FRR_OK) return rf; }   // grows the lists and replays, as often as it takes
        c->proven.add(sig, c->verify_pred);
        return FRR_OK;
    }
    if (c->log.size() >= 4096 && !c->in_replay) return finish(c);   // (a caller that never synchronises: bound the log)
    return FRR_OK;
}

// Synchronisation point: both streams drained, device counters on the host, and -- if a command found a work list too
// small (Counters::first_bad) -- the list grown and the commands from that one onwards replayed, as often as it takes.
// The reference's draw cannot fail (renderer.rs:269-384); neither can this one, short of running out of memory.
int finish(frr_ctx *c)
{
    if (c->in_replay) return FRR_OK;
    int rc = settle(c);
    if (rc != FRR_OK) return rc;
    for (int round = 0;; ++round) {
        if ((rc = drain(c)) != FRR_OK) return rc;
        HIP_TRY(c, hipMemcpy(&c->hc, c->cnt, sizeof(Counters), hipMemcpyDeviceToHost));
        Counters &h = c->hc;
        uint32_t cbm = 0, need_fans = 0; uint64_t worst_bins = 0;
        for (const Lane &L : h.lane) {
            cbm = std::max(cbm, std::max(L.gtab[0].clip_block_max, L.gtab[1].clip_block_max));
            need_fans = std::max(need_fans, std::max(L.gtab[0].need_fans, L.gtab[1].need_fans));
            worst_bins = std::max<uint64_t>(worst_bins, std::max<uint64_t>(L.bin_total, std::max<uint64_t>(L.btab[0].seg_total, L.btab[1].seg_total)));
        }
        c->clip_queue_auto = cbm > (uint32_t)CLIP_QUEUE_AT;
        const uint32_t bad = h.first_bad;
        if (c->host_bad) c->seen_bad = *(volatile uint32_t *)c->host_bad;   // (everything has drained: the word is final)
        if (bad == SEQ_NONE) break;     // (a failure that has been dealt with is reset below)
        size_t i = 0;
        while (i < c->log.size() && c->log[i].seq != bad) ++i;
        // the failed command may belong to a frame whose log is gone (frr_clear came before anybody synchronised): that
        // frame cannot be replayed any more -- and its targets have been cleared since -- but the lists are grown, so that
        // the frames from now on fit
        const bool gone = i == c->log.size();
        if (round == 8) return fail(c, FRR_ERR_CAPACITY, "device work lists still too small after eight replays");
        // grow what was too small
        if (h.overflow & 2u) {
            const uint64_t worst = worst_bins;
            const size_t need = (size_t)(worst + worst / 4 + 1024);
            for (BinSet &B : c->bset) {
                if (!B.bins && (gone || &B != &c->bset[c->log[i].set])) continue;   // (a workspace nobody has used yet is sized when it is)
                if ((rc = ensure(c, B.bins, std::max(need, B.bins.cap()))) != FRR_OK) return rc;
                if ((rc = ensure(c, B.bins2, std::max(need, B.bins2.cap()))) != FRR_OK) return rc;
            }
        }
        if (h.overflow & 1u) {
            const uint64_t nf = need_fans;
            c->fan_hint = std::max<size_t>(c->fan_hint, (size_t)(nf + nf / 8 + 1024));
        }
        // the device tables as they were before the failed command: it has used its own parity's cursors (and, when its
        // block sums were scanned inside the next raster pass's binning launch, that pass has reserved bin space)
        h.first_bad = SEQ_NONE; h.overflow = 0u;
        // (the commands in between that own no table do not count: the "next" command is the next geometry or raster pass)
        for (size_t k = i, seen = 0; k < c->log.size() && seen < 2; ++k) {
            const Cmd &m = c->log[k];
            if (!m.owns_table()) continue;
            ++seen;
            if (m.kind == Cmd::GEOM && k == i) {
                GeomTab &gt = h.lane[m.lane].gtab[m.par];
                for (int r = 0; r < FAN_REGIONS; ++r) gt.fan_cursor[r].v = 0u;
                gt.clip_q = 0u; gt.clip_block_max = 0u; gt.n_emit = 0u; gt.need_fans = 0u;
            } else if (m.kind == Cmd::RASTER) {
                h.lane[m.lane].btab[m.par].seg_total = 0ull; h.lane[m.lane].btab[m.par].ent_cursor = 0u;
            }
        }
        HIP_TRY(c, hipMemcpy(c->cnt, &h, offsetof(Counters, dbg), hipMemcpyHostToDevice));
        if (gone) continue;
        // replay
        std::vector<Cmd> todo(c->log.begin() + (ptrdiff_t)i, c->log.end());
        c->log.resize(i);
        const Bound now = c->fs.bound;
        c->fs = todo[0].pre;
        c->epoch = c->next_seq;
        c->in_replay = true;
        ++c->replays;
        for (const Cmd &m : todo) {
            c->fs.bound = m.pre.bound;   // what the caller set between the commands travels with them
            if ((rc = exec_cmd(c, m)) != FRR_OK) { c->in_replay = false; return rc; }
        }
        c->in_replay = false;
        c->fs.bound = now;
        if ((rc = settle(c)) != FRR_OK) return rc;
    }
    drop_log(c);
    c->epoch = c->next_seq;
    if (c->next_seq > 0xF0000000u) {   // sequence numbers start over (nothing is in flight)
        const uint32_t none = SEQ_NONE;
        HIP_TRY(c, hipMemcpy(&c->cnt.get()->first_bad, &none, sizeof none, hipMemcpyHostToDevice));
        c->next_seq = c->epoch = 1;
    }
    return FRR_OK;
}

// ---- what the entry points share ------------------------------------------------------------------------------------
// a rule of frr_rules.h, answered through the ctx
int rule_rc(frr_ctx *c, const Rule &r) { return r.code == FRR_OK ? FRR_OK : fail(c, r.code, r.msg); }
// pixel_shader_rule with the K a user pixel shader was registered with looked up
int ps_check(frr_ctx *c, VaryingsFrom from, int ps_id, int K)
{
    const UserShader *us = ps_id >= FRR_SHADER_USER_BASE ? user_shader(ps_id) : nullptr;
    return rule_rc(c, pixel_shader_rule(from, ps_id, K, us ? us->K : USER_K_UNKNOWN, c->duni.tex != nullptr));
}
// `who` needs the whole setup list of the latest geometry pass: a frr_draw* on a partitioned ctx keeps only the triangles
// that touch the rank's tile rows of its window (frr_raster of that window and partition alone takes such a list: raster_check)
int need_unfiltered_list(frr_ctx *c, const char *who)
{
    if (!c->fs.geom.read.filter) return FRR_OK;
    return fail(c, FRR_ERR_INVALID, std::string("the setup list of a partitioned frr_draw holds only this rank's triangles; run frr_geometry* (unfiltered) and frr_raster before ") + who);
}
// the common part of a command: its kind, the uniforms and the cull mode at the time of the call, its window
Cmd new_cmd(const frr_ctx *c, Cmd::Kind kind, int32_t x0 = 0, int32_t x1 = 0, int32_t y0 = 0, int32_t y1 = 0)
{
    Cmd cmd;
    cmd.kind = kind; cmd.duni = c->duni; cmd.cull = c->cull;
    cmd.x0 = x0; cmd.x1 = x1; cmd.y0 = y0; cmd.y1 = y1;
    return cmd;
}
// the tail of frr_geometry*: a caller that wants the pass's emission count waits for it (a synchronisation point).  (A pass
// without inputs launches k_geom_empty, whose geom_bookkeeping leaves n_emit = 0: the guard reads the same value.)
int geometry_count(frr_ctx *c, uint64_t *ntris_setup)
{
    if (!ntris_setup) return FRR_OK;
    const int rc = finish(c);
    if (rc != FRR_OK) return rc;
    *ntris_setup = c->fs.geom.read.ntris ? c->hc.lane[c->fs.lane].gtab[c->fs.gpar()].n_emit : 0;
    return FRR_OK;
}
// The host form of a command that writes a caller's buffer (`out`: which field of the command names it): the command runs
// on the temporary device buffer `tmp`, the host waits -- a synchronisation point and, if a list was too small, the replay,
// the command included; the log is empty afterwards -- and `bytes` of `tmp` come back to `host`.  A finish() that failed may
// have left the command in the log: it is purged, so that nothing replays it into the freed buffer.
template <typename T> int host_round_trip(frr_ctx *c, Cmd cmd, T *Cmd::*out, DevBuf<T> &tmp, T *host, size_t bytes, const char *what)
{
    cmd.*out = tmp;
    int rc = exec_cmd(c, cmd);
    const int rf = finish(c);
    if (rc == FRR_OK) rc = rf;
    hipError_t e = hipSuccess;
    if (rc == FRR_OK) e = hipMemcpy(host, tmp, bytes, hipMemcpyDeviceToHost);
    for (size_t k = c->log.size(); k-- > 0;) if (c->log[k].kind == cmd.kind && c->log[k].*out == tmp.get()) c->log.erase(c->log.begin() + (ptrdiff_t)k);
    if (rc != FRR_OK) return rc;
    if (e != hipSuccess) return fail(c, FRR_ERR_HIP, std::string("hipMemcpy ") + what + ": " + hipGetErrorString(e));
    return FRR_OK;
}
// The host form of a shade command (`cmd` with its shader, window and shade_K set): the part of the caller's array the window
// can index becomes a device buffer the ctx owns for as long as the command is logged (frr_ctx::shade_tmp), and the command
// reads that.  shade_K == 0: no copy, a null pointer.
int shade_from_host(frr_ctx *c, Cmd cmd, const float *host_in)
{
    HIP_TRY(c, hipSetDevice(c->device));
    const int K = cmd.shade_K;
    const uint64_t entries = (uint64_t)((int64_t)cmd.y1 - cmd.y0) * (uint64_t)cmd.x1;
    DevBuf<float> tmp;
    if (K > 0) {
        if (tmp.reset((size_t)entries * (size_t)K) != hipSuccess) return nomem(c, "varyings buffer");
        // (returns when the copy is done: in front of the command on any stream)
        HIP_TRY(c, hipMemcpy(tmp, host_in, (size_t)entries * (size_t)K * sizeof(float), hipMemcpyHostToDevice));
    }
    const float *dev = tmp;
    if (K > 0) c->shade_tmp.push_back(std::move(tmp));
    cmd.shade_in = dev; cmd.shade_entries = entries;
    const int rc = exec_cmd(c, cmd);
    // a command that failed on the host is not logged, and nothing will replay it: its copy goes now.  (A synchronisation
    // point inside exec_cmd has dropped log and copies alike.)
    bool logged = false;
    for (size_t k = c->log.size(); k-- > 0 && !logged;) logged = c->log[k].kind == cmd.kind && c->log[k].shade_in == dev;
    if (K > 0 && !logged && !c->shade_tmp.empty() && c->shade_tmp.back().get() == dev) c->shade_tmp.pop_back();
    return rc;
}

} // namespace

extern "C" {

int frr_abi_version(void) { return FRR_ABI_VERSION; }

int frr_vs_input_floats(int vs_id)
{
    switch (vs_id) {
    case FRR_VS_CLIP: return VSInfo<FRR_VS_CLIP>::NF;
    case FRR_VS_CLIP_COLOR: return VSInfo<FRR_VS_CLIP_COLOR>::NF;
    case FRR_VS_PHONG: return VSInfo<FRR_VS_PHONG>::NF;
    case FRR_VS_GOURAUD: return VSInfo<FRR_VS_GOURAUD>::NF;
    }
    if (const UserShader *us = user_shader(vs_id)) return us->nf;
    return FRR_ERR_INVALID;
}
int frr_vs_num_varyings(int vs_id)
{
    switch (vs_id) {
    case FRR_VS_CLIP: return VSInfo<FRR_VS_CLIP>::K;
    case FRR_VS_CLIP_COLOR: return VSInfo<FRR_VS_CLIP_COLOR>::K;
    case FRR_VS_PHONG: return VSInfo<FRR_VS_PHONG>::K;
    case FRR_VS_GOURAUD: return VSInfo<FRR_VS_GOURAUD>::K;
    }
    if (const UserShader *us = user_shader(vs_id)) return us->K;
    return FRR_ERR_INVALID;
}

const char *frr_last_error(const frr_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int frr_create(int device, uint32_t width, uint32_t height, void *stream, frr_ctx **out)
{
    if (!out) return FRR_ERR_INVALID;
    *out = nullptr;
    if (width == 0 || height == 0 || (uint64_t)width * height > 0x3FFFFFFFull) return FRR_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FRR_ERR_HIP;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return FRR_ERR_HIP;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FRR_ERR_HIP; // gfx950 code objects only
    if (hipSetDevice(device) != hipSuccess) return FRR_ERR_HIP;
    frr_ctx *c = new frr_ctx();
    c->device = device; c->W = width; c->H = height;
    if (stream) c->stream = (hipStream_t)stream;
    else { if (acquire_stream(device, &c->stream) != hipSuccess) { delete c; return FRR_ERR_HIP; } c->own_stream = true; }
    const size_t npx = (size_t)width * height;
    c->max_tiles = ((width + TILE - 1) / TILE) * ((height + TILE - 1) / TILE);
    bool ok = ensure_own_set(c, 0) == FRR_OK && c->cnt.reset(1) == hipSuccess && c->zero_texel.reset(16) == hipSuccess;
    for (DevBuf<uint32_t> *b : {&c->tile_counts, &c->tile_offsets, &c->tile_cursor}) ok = ok && b->reset((size_t)c->max_tiles + 1) == hipSuccess;
    for (Event *e : {&c->gset[0].reader.ev, &c->gset[1].reader.ev, &c->bset[0].reader.ev, &c->bset[1].reader.ev, &c->tstream[1].ev, &c->tstream[0].ev,
                     &c->ev_bin[0], &c->ev_bin[1], &c->ev_bin[2], &c->ev_bin[3], &c->ev_join, &c->wire_reader[0].ev, &c->wire_reader[1].ev,
                     &c->ev_verify, &c->ev_export, &c->ev_keep[0], &c->ev_keep[1], &c->ev_keep[2], &c->ev_keep[3]}) ok = ok && e->create() == hipSuccess;
    if (!ok) { frr_destroy(c); return FRR_ERR_NOMEM; }
    c->fs.bound.color = c->own_color[0]; c->fs.bound.depth = c->own_depth[0]; c->fs.bound.tri_id = c->own_tri_id[0];
    // tables of frame 0 (no frame has that number), no failed command
    memset(&c->hc, 0, sizeof c->hc);
    c->hc.first_bad = SEQ_NONE;
    if (hipHostMalloc((void **)&c->host_bad, 64, hipHostMallocMapped) == hipSuccess) {
        *c->host_bad = SEQ_NONE;
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, c->host_bad, 0) == hipSuccess) c->hc.host_bad = (uint32_t *)dp;
    }
    if (hipMemcpy(c->cnt, &c->hc, sizeof(Counters), hipMemcpyHostToDevice) != hipSuccess) { frr_destroy(c); return FRR_ERR_HIP; }
    (void)hipMemsetAsync(c->tile_counts, 0, (c->max_tiles + 1) * 4, c->stream);
    (void)hipMemsetAsync(c->own_color[0], 0, npx * 4, c->stream);      // FrameBuffer::new zero-fills (renderer.rs:423)
    (void)hipMemsetAsync(c->own_depth[0], 0, npx * 4, c->stream);
    (void)hipMemsetAsync(c->own_tri_id[0], 0xFF, npx * 4, c->stream);
    (void)hipMemsetAsync(c->zero_texel, 0, 16, c->stream);
    for (Event &e : c->ev) (void)e.create(true);
    memset(&c->uni, 0, sizeof c->uni);
    frr_set_identity(c->uni.model); frr_set_identity(c->uni.view); frr_set_identity(c->uni.proj);
    c->uni.light_pos[0] = 1.2f; c->uni.light_pos[1] = 1.0f; c->uni.light_pos[2] = 2.0f;   // phong.rs:129
    c->uni.light_color[0] = c->uni.light_color[1] = c->uni.light_color[2] = 1.0f;         // phong.rs:128
    c->uni.ambient_strength = 0.1f; c->uni.specular_strength = 0.5f;                      // phong.rs:131-132
    c->uni.flat_color[0] = c->uni.flat_color[1] = c->uni.flat_color[2] = c->uni.flat_color[3] = 1.0f;
    refresh_dev_uniforms(c);
    if (hipStreamSynchronize(c->stream) != hipSuccess) { frr_destroy(c); return FRR_ERR_HIP; }
    *out = c;
    return FRR_OK;
}

void frr_destroy(frr_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (hipStream_t st : {c->gstream, c->tstream[1].st, c->tstream[0].st, c->stream}) if (st) (void)hipStreamSynchronize(st);
    prof_collect(c);
    for (auto &um : c->user_modules) if (um.second.mod) (void)hipModuleUnload(um.second.mod);
    if (c->host_bad) (void)hipHostFree(c->host_bad);
    // (back to the pool in the reverse order of their typical acquisition, so that the next ctx gets them in the same roles)
    for (hipStream_t st : {c->gstream, c->tstream[0].st, c->tstream[1].st}) release_stream(c->device, st);
    if (c->own_stream) release_stream(c->device, c->stream);
    // Every buffer and event is a member and goes with the ctx, after the synchronisation above: all work that uses one was
    // issued on those four streams, and nothing has been issued since (prof_collect only reads events that have fired).
    delete c;
}

int frr_set_option(frr_ctx *c, const char *name, int64_t v)
{
    if (!c || !name) return FRR_ERR_INVALID;
    { int rc = finish(c); if (rc != FRR_OK) return rc; }   // nothing in flight, nothing to replay under the old setting
    c->proven.clear();                                     // (options change what a pass needs of the lists, or the lists)
    const std::string n(name);
    if (n == "raster_sweep") c->raster_sweep = v != 0;
    else if (n == "raster_nw") { if (v != 0 && v != LIGHT_NW && v != 4 && v != 6 && v != 8 && v != 16) return fail(c, FRR_ERR_INVALID, "raster_nw: 0, 3, 4, 6, 8 or 16"); c->raster_nw = (int)v; }
    else if (n == "raster_occ") { if (v != 0 && v != 4 && v != 6 && v != 8) return fail(c, FRR_ERR_INVALID, "raster_occ: 0, 4, 6 or 8"); c->raster_occ = (int)v; }
    else if (n == "bin_chunks") { if (v < 0) return fail(c, FRR_ERR_INVALID, "bin_chunks >= 0"); c->bin_g = (int)std::min<int64_t>(v, BIN_MAX_G); }
    else if (n == "clear_eager") c->clear_eager = v != 0;
    else if (n == "clip_queue") { if (v < -1 || v > 1) return fail(c, FRR_ERR_INVALID, "clip_queue: -1, 0 or 1"); c->clip_queue = (int)v; }
    else if (n == "tile_slot_records") { if (v < 0 || v > 0x7FFFFFFF) return fail(c, FRR_ERR_INVALID, "tile_slot_records out of range"); c->ent_slot_override = (uint32_t)v; }
    else if (n == "bin_atomics") c->bin_atomics = v != 0;
    else if (n == "bin_capacity") { if (v < 0) return fail(c, FRR_ERR_INVALID, "bin_capacity >= 0"); c->bin_cap_init = (size_t)v; }
    else if (n == "fan_capacity") { if (v < 0) return fail(c, FRR_ERR_INVALID, "fan_capacity >= 0"); c->fan_cap_init = (size_t)v; }
    else if (n == "overlap") { if (v < 0 || v > 2) return fail(c, FRR_ERR_INVALID, "overlap: 0, 1 or 2"); c->overlap = (int)v; }
    else if (n == "bound_targets_in_flight") c->bound_in_flight = v != 0;
    else if (n == "tile_order") { if (v < 0 || v > 2) return fail(c, FRR_ERR_INVALID, "tile_order: 0, 1 or 2"); c->tile_order = (int)v; }
    else if (n == "box_bounds_chunks") { if (v < 0 || v > 1024) return fail(c, FRR_ERR_INVALID, "box_bounds_chunks: 0 .. 1024"); c->box_bounds_chunks = (uint32_t)v; }
    else if (n == "visible_lds_bins") { if (v < 0 || v > (int64_t)VIS_LDS_BINS) return fail(c, FRR_ERR_INVALID, "visible_lds_bins: 0 .. VIS_LDS_BINS"); c->visible_lds_bins = (uint32_t)v; }
    else if (n == "lines_chunk") { if (v < 0 || v > (int64_t)LINES_CHUNK) return fail(c, FRR_ERR_INVALID, "lines_chunk: 0 .. 2^24"); c->lines_chunk = (uint32_t)v; }
    else if (n == "frames_in_flight") { if (v != 1 && v != 2) return fail(c, FRR_ERR_INVALID, "frames_in_flight: 1 or 2"); c->frames_in_flight = (int)v; }
    else return fail(c, FRR_ERR_INVALID, "unknown option");
    return FRR_OK;
}

int frr_set_partition(frr_ctx *c, int rank, int world)
{
    if (!c || world < 1 || rank < 0 || rank >= world) return fail(c, FRR_ERR_INVALID, "bad partition");
    { int rc = settle(c); if (rc != FRR_OK) return rc; } // rows skipped by a fused clear are defined by the old partition
    c->fs.bound.rank = rank; c->fs.bound.world = world;
    return FRR_OK;
}
int frr_set_partition_layout(frr_ctx *c, int blocked)
{
    if (!c) return FRR_ERR_INVALID;
    { int rc = settle(c); if (rc != FRR_OK) return rc; }
    c->fs.bound.part_blocked = blocked != 0;
    return FRR_OK;
}
// owned tile rows of a window of `wh` pixel rows, by the same rule the kernels use (owns_tile_row)
static int owned_band_of(int rank, int world, bool blocked, int64_t wh, int band, int32_t *row0, int32_t *row1)
{
    const int tiles_y = (int)((wh + TILE - 1) / TILE);
    if (world <= 1) {
        if (row0 && band == 0) { *row0 = 0; *row1 = (int32_t)wh; }
        return wh > 0 ? 1 : 0;
    }
    if (blocked) {
        int t0, t1;
        blocked_rows(tiles_y, rank, world, &t0, &t1);
        if (t1 <= t0) return 0;
        if (row0 && band == 0) { *row0 = t0 * TILE; *row1 = (int32_t)std::min<int64_t>(wh, (int64_t)t1 * TILE); }
        return 1;
    }
    const int n = tiles_y > rank ? (tiles_y - rank + world - 1) / world : 0;
    if (row0 && band < n) {
        const int ty = rank + band * world;
        *row0 = ty * TILE; *row1 = (int32_t)std::min<int64_t>(wh, (int64_t)(ty + 1) * TILE);
    }
    return n;
}
static int owned_band(const frr_ctx *c, int64_t wh, int band, int32_t *row0, int32_t *row1)
{
    return owned_band_of(c->fs.bound.rank, c->fs.bound.world, c->fs.bound.part_blocked, wh, band, row0, row1);
}
int frr_partition_rows(int32_t y0, int32_t y1, int rank, int world, int blocked, int32_t band, int32_t *row0, int32_t *row1)
{
    if (y0 > y1 || world < 1 || rank < 0 || rank >= world || band < 0 || (row0 == nullptr) != (row1 == nullptr)) return FRR_ERR_INVALID;
    return owned_band_of(rank, world, blocked != 0, (int64_t)y1 - y0, band, row0, row1);
}
int frr_exchange_plan(int32_t y0, int32_t y1, uint32_t row_elems, int rank, int world, int blocked, int root, frr_xfer *ops, int cap)
{
    if (y0 > y1 || world < 1 || rank < 0 || rank >= world || root < 0 || root >= world || cap < 0 || (cap && !ops)) return FRR_ERR_INVALID;
    const int64_t wh = (int64_t)y1 - y0;
    int n = 0;
    auto put = [&](int kind, int peer, int32_t r0, int32_t r1) {
        if (n < cap) ops[n] = frr_xfer{kind, peer, (uint64_t)r0 * row_elems, (uint64_t)(r1 - r0) * row_elems};
        ++n;
    };
    auto bands_of = [&](int p, int kind, int peer) {
        const int nb = owned_band_of(p, world, blocked != 0, wh, 0, nullptr, nullptr);
        for (int b = 0; b < nb; ++b) {
            int32_t r0 = 0, r1 = 0;
            (void)owned_band_of(p, world, blocked != 0, wh, b, &r0, &r1);
            if (r1 > r0) put(kind, peer, r0, r1);
        }
    };
    if (rank != root) { bands_of(rank, FRR_XFER_SEND, root); return n; }
    for (int p = 0; p < world; ++p) if (p != root) bands_of(p, FRR_XFER_RECV, p);
    bands_of(root, FRR_XFER_COPY, root);
    return n;
}
int frr_owned_band_count(const frr_ctx *c, int32_t y0, int32_t y1)
{
    if (!c || y0 > y1) return FRR_ERR_INVALID;
    return owned_band(c, (int64_t)y1 - y0, 0, nullptr, nullptr);
}
int frr_owned_rows(const frr_ctx *c, int32_t y0, int32_t y1, int32_t band, int32_t *row0, int32_t *row1)
{
    if (!c || y0 > y1 || !row0 || !row1 || band < 0) return FRR_ERR_INVALID;
    int32_t a = 0, b = 0;
    const int n = owned_band(c, (int64_t)y1 - y0, band, &a, &b);
    if (band >= n) return FRR_ERR_INVALID;
    *row0 = a; *row1 = b;
    return FRR_OK;
}
int frr_set_count_fragments(frr_ctx *c, int enable)
{
    if (!c) return FRR_ERR_INVALID;
    c->count_frags = enable != 0;
    return FRR_OK;
}

int frr_bind_targets(frr_ctx *c, void *color, void *depth, void *tri_id)
{
    if (!c) return FRR_ERR_INVALID;
    { int rc = settle(c); if (rc != FRR_OK) return rc; } // a pending clear belongs to the targets bound when it was issued
    if (c->bound_in_flight && (!color || !depth || !tri_id) && (color || depth || tri_id))
        return fail(c, FRR_ERR_INVALID, "option bound_targets_in_flight: bind all three targets, or none (back to the ctx's own)");
    if (!(c->bound_in_flight && !own_targets(c))) { int rc = join_tile_streams(c); if (rc != FRR_OK) return rc; }   // (frames in flight on bound targets: the caller fences)
    if (!color || !depth || !tri_id) {
        // (part of) the ctx's own set: frames on bound targets may have toggled the set index without it ever being allocated
        if (c->bound_in_flight) { int rc = finish(c); if (rc != FRR_OK) return rc; }   // back to own targets: nothing of the bound frames in flight
        int rc = ensure_own_set(c, c->fs.bound.tset);
        if (rc != FRR_OK) return rc;
    }
    Bound &b = c->fs.bound;
    b.color = color ? (uint8_t *)color : c->own_color[b.tset];
    b.depth = depth ? (float *)depth : c->own_depth[b.tset];
    b.tri_id = tri_id ? (uint32_t *)tri_id : c->own_tri_id[b.tset];
    return FRR_OK;
}
int frr_target_ptrs(frr_ctx *c, void **color, void **depth, void **tri_id)
{
    if (!c) return FRR_ERR_INVALID;
    { int rc = settle(c); if (rc != FRR_OK) return rc; } // the caller is about to look at them ...
    { int rc = join_tile_streams(c); if (rc != FRR_OK) return rc; } // ... from its stream
    if (own_targets(c)) { c->exported[c->fs.bound.tset] = true; c->export_stream[c->fs.bound.tset] = c->stream; }   // (frr_clear orders the set's next frame behind those reads)
    if (color) *color = c->fs.bound.color;
    if (depth) *depth = c->fs.bound.depth;
    if (tri_id) *tri_id = c->fs.bound.tri_id;
    return FRR_OK;
}

static int mesh_register(frr_ctx *c, Mesh &&m, uint64_t ntris, int vs, int *mesh_out, uint64_t nverts = 0)
{
    if (m.own_dev) { m.dev = m.own_dev; m.idx = m.own_idx; }
    m.nverts = nverts; m.used = true; m.ntris = ntris; m.vs = vs; m.gen = ++c->mesh_gen;
    *mesh_out = slot_put(c->meshes, std::move(m));
    return FRR_OK;
}
int frr_mesh_upload(frr_ctx *c, const float *vs_inputs, uint64_t ntris, int vs_id, int *mesh_out)
{
    if (!c || !mesh_out || frr_vs_input_floats(vs_id) < 0 || (ntris && !vs_inputs)) return fail(c, FRR_ERR_INVALID, "bad mesh");
    if (ntris >= MAX_PASS_INPUTS) return fail(c, FRR_ERR_UNSUPPORTED, "more than 2^27 triangles per mesh (order keys: 32 per input triangle)");
    HIP_TRY(c, hipSetDevice(c->device));
    Mesh m;
    const int rc = upload(c, m.own_dev, vs_inputs, (size_t)ntris * 3 * frr_vs_input_floats(vs_id) * sizeof(float), "mesh");
    return rc != FRR_OK ? rc : mesh_register(c, std::move(m), ntris, vs_id, mesh_out);
}
int frr_mesh_bind_device(frr_ctx *c, const void *dev, uint64_t ntris, int vs_id, int *mesh_out)
{
    if (!c || !mesh_out || frr_vs_input_floats(vs_id) < 0 || (ntris && !dev)) return fail(c, FRR_ERR_INVALID, "bad mesh");
    if (ntris >= MAX_PASS_INPUTS) return fail(c, FRR_ERR_UNSUPPORTED, "more than 2^27 triangles per mesh (order keys: 32 per input triangle)");
    if (((uintptr_t)dev & 15u) != 0) return fail(c, FRR_ERR_INVALID, "mesh pointer must be 16-byte aligned");
    c->join_epoch += 1;    // the ctx's private streams have to see what the caller's stream wrote into that memory up to now
    Mesh m; m.dev = (const float *)dev;
    return mesh_register(c, std::move(m), ntris, vs_id, mesh_out);
}
// ---- indexed meshes: the Model the reference expands on the CPU (phong.rs:187-205), drawn as it is --------------------
static int indexed_args(frr_ctx *c, const void *verts, uint64_t nverts, const void *idx, uint64_t ntris, int vs_id, int *mesh_out)
{
    if (!c || !mesh_out || frr_vs_input_floats(vs_id) < 0 || (nverts && !verts) || (ntris && !idx)) return fail(c, FRR_ERR_INVALID, "bad mesh");
    if (ntris && !nverts) return fail(c, FRR_ERR_INVALID, "indexed mesh: triangles but no vertices");
    if (ntris >= MAX_PASS_INPUTS) return fail(c, FRR_ERR_UNSUPPORTED, "more than 2^27 triangles per mesh (order keys: 32 per input triangle)");
    if (nverts > 0xFFFFFFFFull) return fail(c, FRR_ERR_UNSUPPORTED, "more than 2^32 - 1 vertices per mesh (u32 indices)");
    return FRR_OK;
}
static int bad_index(frr_ctx *c, uint64_t t, uint64_t nverts)
{
    return fail(c, FRR_ERR_INVALID, "indexed mesh: triangle " + std::to_string(t) + " has an index >= nverts (" + std::to_string(nverts) + "): model.vert(i, j) would panic");
}
int frr_mesh_upload_indexed(frr_ctx *c, const float *vertices, uint64_t nverts, const uint32_t *indices, uint64_t ntris, int vs_id, int *mesh_out)
{
    { int rc = indexed_args(c, vertices, nverts, indices, ntris, vs_id, mesh_out); if (rc != FRR_OK) return rc; }
    if (((uintptr_t)indices & 3u) != 0) return fail(c, FRR_ERR_INVALID, "index pointer must be 4-byte aligned");
    for (uint64_t t = 0; t < ntris; ++t)
        if (indices[3 * t] >= nverts || indices[3 * t + 1] >= nverts || indices[3 * t + 2] >= nverts) return bad_index(c, t, nverts);
    HIP_TRY(c, hipSetDevice(c->device));
    Mesh m; int rc = upload(c, m.own_dev, vertices, (size_t)nverts * frr_vs_input_floats(vs_id) * sizeof(float), "mesh", false);
    // (should the second one fail, the first copy may still be reading `vertices`: the free in m's destructor waits for the device)
    if (rc == FRR_OK) rc = upload(c, m.own_idx, indices, (size_t)ntris * 3 * sizeof(uint32_t), "mesh indices");
    return rc != FRR_OK ? rc : mesh_register(c, std::move(m), ntris, vs_id, mesh_out, nverts);
}
int frr_mesh_bind_device_indexed(frr_ctx *c, const void *dev_vertices, uint64_t nverts, const void *dev_indices, uint64_t ntris, int vs_id, int *mesh_out)
{
    { int rc = indexed_args(c, dev_vertices, nverts, dev_indices, ntris, vs_id, mesh_out); if (rc != FRR_OK) return rc; }
    if (((uintptr_t)dev_vertices & 15u) != 0) return fail(c, FRR_ERR_INVALID, "mesh pointer must be 16-byte aligned");
    if (((uintptr_t)dev_indices & 3u) != 0) return fail(c, FRR_ERR_INVALID, "index pointer must be 4-byte aligned");
    if (ntris) {   // every index < nverts?
        uint32_t bad;
        const int rc = first_bad_on_device(c, &bad, [&](uint32_t *cell) {
            hipLaunchKernelGGL(k_index_check, dim3((uint32_t)std::min<uint64_t>((ntris + 255) / 256, 1024)), dim3(256), 0, c->stream,
                               (const uint32_t *)dev_indices, (uint32_t)ntris, (uint32_t)nverts, cell);
        });
        if (rc != FRR_OK) return rc;
        if (bad != 0xFFFFFFFFu) return bad_index(c, bad, nverts);
    }
    c->join_epoch += 1;    // the ctx's private streams have to see what the caller's stream wrote into that memory up to now
    Mesh m; m.dev = (const float *)dev_vertices; m.idx = (const uint32_t *)dev_indices;
    return mesh_register(c, std::move(m), ntris, vs_id, mesh_out, nverts);
}
int frr_mesh_free(frr_ctx *c, int mesh)
{
    if (!c || !slot_ok(c->meshes, mesh)) return fail(c, FRR_ERR_INVALID, "bad mesh id");
    { int rc = finish(c); if (rc != FRR_OK) return rc; }   // nothing reads it any more, nothing will replay a draw of it
    for (DrawList &l : c->lists)   // a list that names it holds its pointers: dead from now on, whoever gets the id next
        for (size_t i = 0; l.used && !l.dead && i < l.mesh.size(); ++i)
            if (l.mesh[i] == mesh && l.mesh_gen[i] == c->meshes[mesh].gen) l.dead = true;
    c->meshes[mesh] = Mesh();   // (frees the library's copies)
    return FRR_OK;
}

// ---- draw_line (renderer.rs:540-588): lists of segments and the wireframe of the latest setup list ------------------
static int bad_segment(frr_ctx *c, uint64_t k)
{
    return fail(c, FRR_ERR_INVALID, "lines: segment " + std::to_string(k) + " would write past the " + std::to_string(c->W) + " x " + std::to_string(c->H) +
                                    " buffer: set_pixel would panic (renderer.rs:497-503)");
}
static int lines_args(frr_ctx *c, const void *xyxy, const void *rgba, uint64_t nlines, int *lines_out)
{
    if (!c || !lines_out || (nlines && (!xyxy || !rgba))) return fail(c, FRR_ERR_INVALID, "bad line list");
    if (nlines >= (1ull << 31)) return fail(c, FRR_ERR_UNSUPPORTED, "2^31 or more segments per list (owner numbers are u32)");
    return FRR_OK;
}
static int lines_register(frr_ctx *c, Lines &&l, uint64_t n, int *lines_out)
{
    if (l.own_xyxy) { l.xyxy = l.own_xyxy; l.rgba = l.own_rgba; }
    l.n = n; l.used = true;
    *lines_out = slot_put(c->lines, std::move(l));
    return FRR_OK;
}
int frr_lines_upload(frr_ctx *c, const uint32_t *xyxy, const uint8_t *rgba, uint64_t nlines, int *lines_out)
{
    { int rc = lines_args(c, xyxy, rgba, nlines, lines_out); if (rc != FRR_OK) return rc; }
    const uint64_t npix = (uint64_t)c->W * c->H;
    for (uint64_t k = 0; k < nlines; ++k)
        if (line_max_index(line_setup(xyxy[4 * k], xyxy[4 * k + 1], xyxy[4 * k + 2], xyxy[4 * k + 3]), c->W) >= npix) return bad_segment(c, k);
    HIP_TRY(c, hipSetDevice(c->device));
    Lines l; int rc = upload(c, l.own_xyxy, xyxy, (size_t)nlines * 16, "lines", false);
    if (rc == FRR_OK) rc = upload(c, l.own_rgba, rgba, (size_t)nlines * 4, "line colours");   // (on failure l's destructor waits, as for an indexed mesh)
    return rc != FRR_OK ? rc : lines_register(c, std::move(l), nlines, lines_out);
}
int frr_lines_bind_device(frr_ctx *c, const void *dev_xyxy, const void *dev_rgba, uint64_t nlines, int *lines_out)
{
    { int rc = lines_args(c, dev_xyxy, dev_rgba, nlines, lines_out); if (rc != FRR_OK) return rc; }
    if (((uintptr_t)dev_xyxy & 15u) != 0) return fail(c, FRR_ERR_INVALID, "segment pointer must be 16-byte aligned");
    if (((uintptr_t)dev_rgba & 3u) != 0) return fail(c, FRR_ERR_INVALID, "colour pointer must be 4-byte aligned");
    if (nlines) {   // does every walk stay inside the buffer?
        uint32_t bad;
        const int rc = first_bad_on_device(c, &bad, [&](uint32_t *cell) {
            hipLaunchKernelGGL(k_lines_check, dim3((uint32_t)std::min<uint64_t>((nlines + 255) / 256, 1024)), dim3(256), 0, c->stream,
                               (const uint4 *)dev_xyxy, (uint32_t)nlines, c->W, (uint64_t)c->W * c->H, cell);
        });
        if (rc != FRR_OK) return rc;
        if (bad != 0xFFFFFFFFu) return bad_segment(c, bad);
    }
    Lines l; l.xyxy = (const uint4 *)dev_xyxy; l.rgba = (const uint32_t *)dev_rgba;
    return lines_register(c, std::move(l), nlines, lines_out);   // (the host wait above stands for a join of the ctx's private streams)
}
int frr_lines_free(frr_ctx *c, int lines)
{
    if (!c || !slot_ok(c->lines, lines)) return fail(c, FRR_ERR_INVALID, "bad line list id");
    { int rc = finish(c); if (rc != FRR_OK) return rc; }   // nothing reads it any more, nothing will replay a draw of it
    c->lines[lines] = Lines();   // (frees the library's copies)
    return FRR_OK;
}
int frr_draw_lines(frr_ctx *c, int lines)
{
    if (!c || !slot_ok(c->lines, lines)) return fail(c, FRR_ERR_INVALID, "bad line list id");
    if (c->lines[lines].n == 0) return FRR_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    Cmd cmd = new_cmd(c, Cmd::LINES);
    cmd.lines = lines;
    return exec_cmd(c, cmd);
}
int frr_draw_wireframe(frr_ctx *c, const uint8_t rgba[4])
{
    if (!c || !rgba) return fail(c, FRR_ERR_INVALID, "bad arguments");
    const FrameState &f = c->fs;
    if (f.geom.none()) return fail(c, FRR_ERR_INVALID, "frr_draw_wireframe before frr_geometry");
    { const int rc = need_unfiltered_list(c, "frr_draw_wireframe"); if (rc != FRR_OK) return rc; }
    if (f.geom.read.ntris == 0) return FRR_OK;
    // (segment numbers + 1 are u32, and a wave's last batch of 64 must not wrap either)
    if (3ull * (f.geom.read.ntris + f.geom.fan_cap) + 64ull >= 0xFFFFFFFFull) return fail(c, FRR_ERR_UNSUPPORTED, "wireframe: more than 2^32 / 3 setup slots (owner numbers are u32)");
    HIP_TRY(c, hipSetDevice(c->device));
    Cmd cmd = new_cmd(c, Cmd::LINES);
    cmd.lines = -1;
    memcpy(&cmd.wire_rgba, rgba, 4);
    return exec_cmd(c, cmd);
}
int64_t frr_host_line_pixels(uint32_t x1, uint32_t y1, uint32_t x2, uint32_t y2, uint32_t width, uint64_t *out, uint64_t cap)
{
    const LineSeg s = line_setup(x1, y1, x2, y2);
    const uint64_t n = line_iters(s);
    uint64_t count = 0;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t p[2];
        const int np = line_iter(s, (uint32_t)i, width, p);
        for (int w = 0; w < np; ++w, ++count) if (out && count < cap) out[count] = p[w];
    }
    return (int64_t)count;
}

int frr_texture_upload(frr_ctx *c, int slot, const uint8_t *rgba, uint32_t w, uint32_t h)
{
    if (!c || slot < 0 || slot >= FRR_MAX_TEXTURES || !rgba || w == 0 || h == 0) return fail(c, FRR_ERR_INVALID, "bad texture");
    if (h < w) return fail(c, FRR_ERR_UNSUPPORTED, "texture height < width: sample_2d clamps y with width (renderer.rs:523) and would index out of bounds");
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = finish(c); if (rc != FRR_OK) return rc; }   // the draws issued so far sample the old texture
    c->tex_epoch += 1;                                     // ... and a user VS may sample it: no pass is proven for the new one
    Texture &t = c->tex[slot];   // (changed -- pointer, width and height together -- only once the new texels are on the device)
    { int rc = upload(c, t.dev, rgba, (size_t)w * h * 4, "texture"); if (rc != FRR_OK) return rc; }
    t.w = w; t.h = h;
    refresh_dev_uniforms(c);
    return FRR_OK;
}

int frr_set_uniforms(frr_ctx *c, const frr_uniforms *u)
{
    if (!c || !u) return FRR_ERR_INVALID;
    c->uni = *u;
    refresh_dev_uniforms(c);
    return FRR_OK;
}

int frr_set_user_uniforms(frr_ctx *c, const float *values, int n)
{
    if (!c || n < 0 || n > FRR_MAX_USER_UNIFORMS || (n && !values)) return fail(c, FRR_ERR_INVALID, "user uniforms: at most FRR_MAX_USER_UNIFORMS floats");
    memset(c->duni.user, 0, sizeof c->duni.user);
    if (n) memcpy(c->duni.user, values, (size_t)n * sizeof(float));
    return FRR_OK;
}

int frr_set_cull(frr_ctx *c, int mode)
{
    if (!c) return FRR_ERR_INVALID;
    if (mode != FRR_CULL_NONE && mode != FRR_CULL_NEG && mode != FRR_CULL_POS) return fail(c, FRR_ERR_INVALID, "unknown cull mode (FRR_CULL_NONE, FRR_CULL_NEG, FRR_CULL_POS)");
    c->cull = mode;
    return FRR_OK;
}

int frr_shader_register(frr_ctx *c, const char *hip_source, int vs_input_floats, int num_varyings, int *shader_id)
{
    if (!hip_source || !shader_id || vs_input_floats < 1 || vs_input_floats > 64 || num_varyings < 0 || num_varyings > FRR_MAX_VARYINGS)
        return fail(c, FRR_ERR_INVALID, "bad shader description (1..64 input floats, 0..FRR_MAX_VARYINGS varyings)");
    // the program: fixed-width types (hiprtc keeps them in a namespace), this shader's shape, the device header, the
    // user's functions, the kernels -- the very headers libfrr_hip.so itself was built from
    std::string src = "using __hip_internal::int8_t; using __hip_internal::uint8_t; using __hip_internal::int16_t; using __hip_internal::uint16_t;\n"
                      "using __hip_internal::int32_t; using __hip_internal::uint32_t; using __hip_internal::int64_t; using __hip_internal::uint64_t;\n"
                      "typedef unsigned long uintptr_t;\n#define FRR_USER_SHADER 1\n";
    src += "#define FRR_USER_NF " + std::to_string(vs_input_floats) + "\n#define FRR_USER_K " + std::to_string(num_varyings) + "\n";
    src += "#include \"frr_device.h\"\n#line 1 \"user_shader\"\n";
    src += hip_source;
    src += "\n#include \"frr_kernels.h\"\n#include \"frr_shade.h\"\n";
    const char *hdr_txt[] = {frr_src_device_h, frr_src_exact_h, frr_src_kernels_h, frr_src_raster_h, frr_src_shade_h, frr_src_visible_h, frr_src_frr_h};
    const char *hdr_name[] = {"frr_device.h", "frr_exact.h", "frr_kernels.h", "frr_raster.h", "frr_shade.h", "frr_visible.h", "../../include/frr.h"};
    hiprtcProgram prog = nullptr;
    if (hiprtcCreateProgram(&prog, src.c_str(), "frr_user_program.hip", 7, hdr_txt, hdr_name) != HIPRTC_SUCCESS) return fail(c, FRR_ERR_HIP, "hiprtcCreateProgram");
    UserShader *us = new UserShader();
    us->nf = vs_input_floats; us->K = num_varyings;
    const std::string U = std::to_string(FRR_SHADER_USER_BASE), Ks = std::to_string(num_varyings);
    std::vector<std::string> exprs = {"frr::k_geom_single<" + U + ", false>", "frr::k_geom_clip<" + U + ", false>"};
    const std::string geom_idx_expr = "frr::k_geom_single<" + U + ", true>", clip_idx_expr = "frr::k_geom_clip<" + U + ", true>";   // indexed meshes
    (void)hiprtcAddNameExpression(prog, geom_idx_expr.c_str());
    (void)hiprtcAddNameExpression(prog, clip_idx_expr.c_str());
    std::string geom_inst_expr[2], clip_inst_expr[2];   // instanced passes ([indexed mesh])
    for (int idx = 0; idx < 2; ++idx) {
        geom_inst_expr[idx] = "frr::k_geom_single<" + U + (idx ? ", true, true>" : ", false, true>");
        clip_inst_expr[idx] = "frr::k_geom_clip<" + U + (idx ? ", true, true>" : ", false, true>");
        (void)hiprtcAddNameExpression(prog, geom_inst_expr[idx].c_str());
        (void)hiprtcAddNameExpression(prog, clip_inst_expr[idx].c_str());
    }
    const std::string geom_list_expr = "frr::k_geom_single<" + U + ", false, true, true>", clip_list_expr = "frr::k_geom_clip<" + U + ", false, true, true>";   // list passes
    (void)hiprtcAddNameExpression(prog, geom_list_expr.c_str());
    (void)hiprtcAddNameExpression(prog, clip_list_expr.c_str());
    const std::string sweep_expr = "frr::k_raster<" + Ks + ", " + U + ">";   // the brute-force tile kernel (option raster_sweep)
    (void)hiprtcAddNameExpression(prog, sweep_expr.c_str());
    const std::string entries_expr = "frr::k_raster_entries<" + Ks + ", " + U + ">";   // windows whose rows share depth entries (x0 < 0)
    (void)hiprtcAddNameExpression(prog, entries_expr.c_str());
    // frr_shade_varyings (frr_shade.h): scalar loads, and -- where K allows them -- 16-byte loads
    const bool shade_vec = num_varyings > 0 && num_varyings % 4 == 0;
    const std::string shade_expr[2] = {"frr::k_shade_vary<" + Ks + ", " + U + ", false>", "frr::k_shade_vary<" + Ks + ", " + U + ", true>"};
    const std::string shade_items_expr[2] = {"frr::k_shade_items<" + Ks + ", " + U + ", false>", "frr::k_shade_items<" + Ks + ", " + U + ", true>"};   // frr_shade_items
    for (int vec = 0; vec < (shade_vec ? 2 : 1); ++vec) { (void)hiprtcAddNameExpression(prog, shade_expr[vec].c_str()); (void)hiprtcAddNameExpression(prog, shade_items_expr[vec].c_str()); }
    for (int cnt = 0; cnt < 2; ++cnt)
        for (int sh = 0; sh < 6; ++sh)
            exprs.push_back("frr::k_raster_span<" + Ks + ", " + U + ", " + (cnt ? "true" : "false") + ", " + std::to_string(kSpanShapes[sh][0]) + ", " + std::to_string(kSpanShapes[sh][1]) + ">");
    for (const std::string &e : exprs) (void)hiprtcAddNameExpression(prog, e.c_str());
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-Wno-unused-function"};
    const hiprtcResult res = hiprtcCompileProgram(prog, 7, opts);
    if (res != HIPRTC_SUCCESS) {
        size_t n = 0;
        (void)hiprtcGetProgramLogSize(prog, &n);
        std::string log(n + 1, '\0');
        if (n) (void)hiprtcGetProgramLog(prog, &log[0]);
        (void)hiprtcDestroyProgram(&prog);
        delete us;
        return fail(c, FRR_ERR_UNSUPPORTED, std::string("user shader does not compile:\n") + log.c_str());
    }
    bool ok = true;
    auto lowered = [&](const std::string &e) { const char *n = nullptr; ok = ok && hiprtcGetLoweredName(prog, e.c_str(), &n) == HIPRTC_SUCCESS && n; return std::string(n ? n : ""); };
    us->geom = lowered(exprs[0]); us->clip = lowered(exprs[1]); us->geom_idx = lowered(geom_idx_expr); us->clip_idx = lowered(clip_idx_expr); us->sweep = lowered(sweep_expr); us->entries = lowered(entries_expr);
    for (int idx = 0; idx < 2; ++idx) { us->geom_inst[idx] = lowered(geom_inst_expr[idx]); us->clip_inst[idx] = lowered(clip_inst_expr[idx]); }
    us->geom_list = lowered(geom_list_expr); us->clip_list = lowered(clip_list_expr);
    for (int vec = 0; vec < (shade_vec ? 2 : 1); ++vec) { us->shade[vec] = lowered(shade_expr[vec]); us->shade_items[vec] = lowered(shade_items_expr[vec]); }
    for (int cnt = 0; cnt < 2; ++cnt)
        for (int sh = 0; sh < 6; ++sh) us->span[cnt][sh] = lowered(exprs[2 + (size_t)cnt * 6 + sh]);
    size_t cs = 0;
    ok = ok && hiprtcGetCodeSize(prog, &cs) == HIPRTC_SUCCESS && cs;
    if (ok) { us->code.resize(cs); ok = hiprtcGetCode(prog, us->code.data()) == HIPRTC_SUCCESS; }
    (void)hiprtcDestroyProgram(&prog);
    if (!ok) { delete us; return fail(c, FRR_ERR_HIP, "hiprtc: no code object"); }
    std::lock_guard<std::mutex> lk(g_shader_mu);
    g_shaders.push_back(us);
    *shader_id = FRR_SHADER_USER_BASE + (int)g_shaders.size() - 1;
    return FRR_OK;
}

int frr_clear(frr_ctx *c, const uint8_t rgba[4], float depth)
{
    if (!c || !rgba) return FRR_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    uint32_t packed;
    memcpy(&packed, rgba, 4);
    FrameState &f = c->fs;
    // Has a command failed since the host last looked (a word the device writes into host memory: no synchronisation)?
    // Then repair now -- replay the frame if its log is still here, grow the lists either way -- before this frame goes on.
    if (c->host_bad && *(volatile uint32_t *)c->host_bad != c->seen_bad) { const int rc = finish(c); if (rc != FRR_OK) return rc; }
    // A new frame: the commands logged so far are history.  (One of them may have failed unseen: it and everything after
    // it left the targets untouched, and they are overwritten now.  Device statistics are tagged with the frame number.)
    drop_log(c);
    c->epoch = c->next_seq;
    c->replays = 0;
    f.frame_no += 1;
    f.tris_in = 0; f.draws = 0;
    f.geom.setup_list_gone();        // (of a preceding frr_geometry)
    f.geom.scan_pending = false;
    f.clear.unowned_debt = false;    // superseded: the clear covers every row
    if (c->frames_in_flight == 2 && own_targets(c)) {
        // own targets: this frame takes the other set (and its tile kernels the other stream), so that it need not wait
        // for the previous frame's tile kernel to drain; the old set's content is dead (the clear overwrites everything)
        const int t = f.bound.tset ^ 1;
        { const int rc = ensure_own_set(c, t); if (rc != FRR_OK) return rc; }
        if (!c->tstream[1].st && acquire_stream(c->device, &c->tstream[1].st) != hipSuccess) return fail(c, FRR_ERR_HIP, "frame stream");
        f.bound.tset = t;
        f.bound.color = c->own_color[t]; f.bound.depth = c->own_depth[t]; f.bound.tri_id = c->own_tri_id[t];
        f.lane = t;    // ... and its own device tables: nothing the two frames' bookkeeping threads write is shared
    } else if (frames_alternate(c)) {
        // caller-bound targets, option bound_targets_in_flight: the caller has bound another target set for this frame;
        // the frame takes the other private stream, workspace set and lane
        bool ok = (c->tstream[1].st || acquire_stream(c->device, &c->tstream[1].st) == hipSuccess) &&
                  (c->tstream[0].st || acquire_stream(c->device, &c->tstream[0].st) == hipSuccess);
        if (!ok) return fail(c, FRR_ERR_HIP, "frame streams");
        f.bound.tset ^= 1;
        f.lane = f.bound.tset;
    } else {
        f.lane = 0;
    }
    if (own_targets(c) && c->exported[f.bound.tset]) {
        // The pointers of this own target set were handed out (frr_target_ptrs / frr_frame_fence) when it last held a frame:
        // what the caller has queued on that stream since -- its reads of that frame -- comes before this frame's writes.
        // (Same stream: in order anyway.  Only callers that take the pointers pay for the event.)
        c->exported[f.bound.tset] = false;
        hipStream_t ts = tstream_of(c);
        if (c->export_stream[f.bound.tset] != ts) {
            HIP_TRY(c, hipEventRecord(c->ev_export, c->export_stream[f.bound.tset]));
            HIP_TRY(c, hipStreamWaitEvent(ts, c->ev_export, 0));
        }
    }
    if (c->clear_eager) { f.clear.pending = false; return clear_now(c, packed, depth, true); }
    f.clear.rgba = packed; f.clear.depth = depth;
    f.clear.pending = true;
    f.clear.wait_serial = c->wait_serial;
    return FRR_OK;
}

int frr_geometry(frr_ctx *c, int mesh, uint64_t *ntris_setup)
{
    if (!c || !slot_ok(c->meshes, mesh)) return fail(c, FRR_ERR_INVALID, "bad mesh id");
    HIP_TRY(c, hipSetDevice(c->device));
    Cmd cmd = new_cmd(c, Cmd::GEOM);
    cmd.mesh = mesh;
    const int rc = exec_cmd(c, cmd);
    return rc != FRR_OK ? rc : geometry_count(c, ntris_setup);
}

// ---- instanced passes: one mesh under a table of model matrices (the loop over objects of phong.rs:319-331) ----------
static int instances_register(frr_ctx *c, Instances &&t, uint64_t ninst, int *inst_out)
{
    if (t.own) t.dev = t.own;
    t.n = ninst; t.used = true; t.gen = ++c->inst_gen;
    *inst_out = slot_put(c->instances, std::move(t));
    return FRR_OK;
}
int frr_instances_upload(frr_ctx *c, const float *models, uint64_t ninst, int *inst_out)
{
    if (!c || !inst_out || (ninst && !models)) return fail(c, FRR_ERR_INVALID, "bad instance table");
    if (ninst >= MAX_PASS_INPUTS) return fail(c, FRR_ERR_UNSUPPORTED, "2^27 instances or more (order keys: 32 per input triangle of a pass)");
    HIP_TRY(c, hipSetDevice(c->device));
    Instances t;
    if (ninst) { const int rc = upload(c, t.own, models, (size_t)ninst * 16 * sizeof(float), "instance table"); if (rc != FRR_OK) return rc; }
    return instances_register(c, std::move(t), ninst, inst_out);
}
int frr_instances_bind_device(frr_ctx *c, const void *dev_models, uint64_t ninst, int *inst_out)
{
    if (!c || !inst_out || (ninst && !dev_models)) return fail(c, FRR_ERR_INVALID, "bad instance table");
    if (ninst >= MAX_PASS_INPUTS) return fail(c, FRR_ERR_UNSUPPORTED, "2^27 instances or more (order keys: 32 per input triangle of a pass)");
    if (((uintptr_t)dev_models & 15u) != 0) return fail(c, FRR_ERR_INVALID, "instance table pointer must be 16-byte aligned");
    c->join_epoch += 1;    // the ctx's private streams have to see what the caller's stream wrote into that memory up to now
    Instances t; t.dev = (const float *)dev_models;
    return instances_register(c, std::move(t), ninst, inst_out);
}
int frr_instances_free(frr_ctx *c, int inst)
{
    if (!c || !slot_ok(c->instances, inst)) return fail(c, FRR_ERR_INVALID, "bad instance table id");
    { int rc = finish(c); if (rc != FRR_OK) return rc; }   // nothing reads it any more, nothing will replay a pass over it
    c->instances[inst] = Instances();
    return FRR_OK;
}
// the GEOM command of an instanced pass, checked: nothing is allocated for a pass that is refused
static int instanced_cmd(frr_ctx *c, int mesh, int inst, Cmd *cmd)
{
    if (!c || !slot_ok(c->meshes, mesh)) return fail(c, FRR_ERR_INVALID, "bad mesh id");
    if (!slot_ok(c->instances, inst)) return fail(c, FRR_ERR_INVALID, "bad instance table id");
    const uint64_t ntris = c->meshes[mesh].ntris, ninst = c->instances[inst].n;
    if (ntris && ninst && ntris * ninst >= MAX_PASS_INPUTS)   // (both factors are below 2^27: no wrap)
        return fail(c, FRR_ERR_UNSUPPORTED, "2^27 (instance, triangle) pairs or more in one pass (order keys: 32 per input triangle)");
    HIP_TRY(c, hipSetDevice(c->device));
    *cmd = new_cmd(c, Cmd::GEOM);
    cmd->mesh = mesh; cmd->inst = inst;
    h_mat4_mul(c->uni.proj, c->uni.view, cmd->pv);   // as refresh_dev_uniforms builds u.mvp
    return FRR_OK;
}
int frr_geometry_instanced(frr_ctx *c, int mesh, int inst, uint64_t *ntris_setup)
{
    Cmd cmd;
    int rc = instanced_cmd(c, mesh, inst, &cmd);
    if (rc != FRR_OK || (rc = exec_cmd(c, cmd)) != FRR_OK) return rc;
    return geometry_count(c, ntris_setup);
}
void frr_host_instance_mvp(const float proj[16], const float view[16], const float model[16], float out[16])
{
    float pv[16];
    h_mat4_mul(proj, view, pv);
    h_mat4_mul(pv, model, out);
}

// ---- draw lists: many meshes under their own matrices in one pass (the whole setup loop of phong.rs:319-359) ---------
int frr_drawlist_upload(frr_ctx *c, const frr_draw_item *items, uint64_t nitems, int *list_out)
{
    if (!c || !list_out || (nitems && !items)) return fail(c, FRR_ERR_INVALID, "bad draw list");
    if (nitems >= MAX_PASS_INPUTS) return fail(c, FRR_ERR_UNSUPPORTED, "2^27 items or more in one draw list");
    uint64_t total = 0;
    for (uint64_t i = 0; i < nitems; ++i) {
        const std::string who = "draw list: item " + std::to_string(i);
        if (items[i].reserved != 0) return fail(c, FRR_ERR_INVALID, who + ": reserved must be 0");
        if (!slot_ok(c->meshes, items[i].mesh)) return fail(c, FRR_ERR_INVALID, who + ": bad mesh id");
        if (c->meshes[items[i].mesh].vs != c->meshes[items[0].mesh].vs)
            return fail(c, FRR_ERR_INVALID, who + ": its mesh's vertex shader is not item 0's (one vertex shader per list)");
        total += c->meshes[items[i].mesh].ntris;   // (each below 2^27, fewer than 2^27 of them: no wrap)
    }
    if (total >= MAX_PASS_INPUTS) return fail(c, FRR_ERR_UNSUPPORTED, "2^27 triangles or more in one draw list (order keys: 32 per input triangle of a pass)");
    HIP_TRY(c, hipSetDevice(c->device));
    DrawList l;
    std::vector<ListRow> rows(nitems);
    std::vector<uint32_t> first(2 * nitems);
    std::vector<float> models(16 * nitems);
    l.mesh.resize(nitems); l.mesh_gen.resize(nitems);
    uint32_t at = 0;
    for (uint64_t i = 0; i < nitems; ++i) {
        const Mesh &m = c->meshes[items[i].mesh];
        rows[i] = ListRow{m.dev, m.idx, (uint32_t)m.nverts, (uint32_t)m.ntris, at, 0u};
        first[i] = at; first[nitems + i] = (uint32_t)m.ntris;
        at += (uint32_t)m.ntris;
        memcpy(&models[16 * i], items[i].model, sizeof items[i].model);
        l.mesh[i] = items[i].mesh; l.mesh_gen[i] = m.gen;
        l.any_dev = l.any_dev || !m.own_dev;
    }
    if (nitems) {
        l.vs = c->meshes[items[0].mesh].vs;
        int rc = upload(c, l.rows, rows.data(), rows.size() * sizeof(ListRow), "draw list", false);
        if (rc == FRR_OK) rc = upload(c, l.first, first.data(), first.size() * sizeof(uint32_t), "draw list", false);
        // (the last one waits for all three; should one fail, the frees in l's destructor wait for the device)
        if (rc == FRR_OK) rc = upload(c, l.models, models.data(), models.size() * sizeof(float), "draw list");
        if (rc != FRR_OK) return rc;
    }
    l.hrows = std::move(rows);
    l.n = nitems; l.total = total; l.used = true; l.gen = ++c->list_gen;
    *list_out = slot_put(c->lists, std::move(l));
    return FRR_OK;
}
int frr_drawlist_free(frr_ctx *c, int list)
{
    if (!c || !slot_ok(c->lists, list)) return fail(c, FRR_ERR_INVALID, "bad draw list id");
    { int rc = finish(c); if (rc != FRR_OK) return rc; }   // nothing reads it any more, nothing will replay a pass over it
    c->lists[list] = DrawList();
    return FRR_OK;
}
// the GEOM command of a list pass, checked
static int list_cmd(frr_ctx *c, int list, Cmd *cmd)
{
    if (!c || !slot_ok(c->lists, list)) return fail(c, FRR_ERR_INVALID, "bad draw list id");
    if (c->lists[list].dead) return fail(c, FRR_ERR_INVALID, "a mesh the draw list names was freed: the list is dead (frr_drawlist_free still takes it)");
    HIP_TRY(c, hipSetDevice(c->device));
    *cmd = new_cmd(c, Cmd::GEOM);
    cmd->list = list; cmd->list_gen = c->lists[list].gen;
    h_mat4_mul(c->uni.proj, c->uni.view, cmd->pv);   // as refresh_dev_uniforms builds u.mvp
    return FRR_OK;
}
int frr_geometry_list(frr_ctx *c, int list, uint64_t *ntris_setup)
{
    Cmd cmd;
    int rc = list_cmd(c, list, &cmd);
    if (rc != FRR_OK || (rc = exec_cmd(c, cmd)) != FRR_OK) return rc;
    return geometry_count(c, ntris_setup);
}
// the GEOM command of a predicated list pass, checked: the list as frr_draw_list checks it, then the keep rule
static int list_if_cmd(frr_ctx *c, int list, const void *dev_keep_u32, uint64_t keep_entries, uint32_t min_value, Cmd *cmd)
{
    int rc = list_cmd(c, list, cmd);
    if (rc == FRR_OK) rc = rule_rc(c, keep_rule(dev_keep_u32, keep_entries, c->lists[list].n));
    if (rc != FRR_OK) return rc;
    cmd->pred = true; cmd->keep = (const uint32_t *)dev_keep_u32; cmd->keep_entries = keep_entries; cmd->min_value = min_value;
    return FRR_OK;
}
int frr_geometry_list_if(frr_ctx *c, int list, const void *dev_keep_u32, uint64_t keep_entries, uint32_t min_value, uint64_t *ntris_setup)
{
    Cmd cmd;
    int rc = list_if_cmd(c, list, dev_keep_u32, keep_entries, min_value, &cmd);
    if (rc != FRR_OK || (rc = exec_cmd(c, cmd)) != FRR_OK) return rc;
    return geometry_count(c, ntris_setup);
}
int frr_geometry_item_ranges(frr_ctx *c, uint32_t *id_first, uint32_t *id_count, uint64_t cap, uint64_t *nitems)
{
    if (!c || !nitems || c->fs.geom.none()) return fail(c, FRR_ERR_INVALID, "no geometry pass to take item ranges from");
    { const int rc = need_unfiltered_list(c, "frr_geometry_item_ranges"); if (rc != FRR_OK) return rc; }
    { int rcs = finish(c); if (rcs != FRR_OK) return rcs; }
    const FrameState &f = c->fs;
    const GeomTab &gt = c->hc.lane[f.lane].gtab[f.gpar()];
    const GeomSet &S = c->gset[f.geom.set];
    const uint64_t n = f.geom.nitems, w = std::min(cap, n);
    const uint32_t *item_first = nullptr;
    { const int rc = list_item_first(c, &item_first); if (rc != FRR_OK) return rc; }
    *nitems = n;
    if (!w || (!id_first && !id_count)) return FRR_OK;
    const uint32_t nt = (uint32_t)f.geom.read.ntris, n_emit = nt ? gt.n_emit : 0u;
    { int rc = ensure(c, c->item_tmp, (size_t)n + 1); if (rc != FRR_OK) return rc; }
    hipLaunchKernelGGL(k_item_firsts, dim3((uint32_t)((n + 256) / 256)), dim3(256), 0, c->stream, item_first, (uint32_t)f.geom.stride, (uint32_t)n, nt,
                       S.tinfo.get(), S.block_prefix.get(), n_emit, c->item_tmp.get());
    HIP_TRY(c, hipGetLastError());
    std::vector<uint32_t> e(w + 1);
    HIP_TRY(c, hipMemcpyAsync(e.data(), c->item_tmp.get(), (w + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (uint64_t i = 0; i < w; ++i) {
        if (id_first) id_first[i] = gt.tri_base + e[i];
        if (id_count) id_count[i] = e[i + 1] - e[i];
    }
    return FRR_OK;
}
int64_t frr_host_list_item(const uint32_t *first, const uint32_t *ntris, uint64_t nitems, uint32_t t)
{
    if (!first || !ntris || nitems > 0xFFFFFFFFull) return -1;
    const uint32_t i = list_item_search(first, ntris, 0u, (uint32_t)nitems, t);
    return i < nitems && first[i] <= t ? (int64_t)i : -1;
}

// argument checks of frr_raster; *nothing: the call is valid and draws nothing
static int raster_check(frr_ctx *c, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1, bool *nothing)
{
    const FrameState &f = c->fs;
    if (f.geom.none()) return fail(c, FRR_ERR_INVALID, "frr_raster before frr_geometry");
    int rc = rule_rc(c, window_rule(WINDOW_RASTER, c->W, c->H, x0, x1, y0, y1));
    // the mesh's vertex shader -- the same user shader, another one, or a built-in -- has to hand the pixel shader its varyings.
    // A list without items has no vertex shader (DrawList::vs is a placeholder): K_OF_NOTHING, as in draw_pass.
    const bool no_vs = f.geom.read.list >= 0 && f.geom.nitems == 0;
    if (rc == FRR_OK) rc = ps_check(c, no_vs ? K_OF_NOTHING : K_OF_GEOMETRY, ps_id, frr_vs_num_varyings(f.geom.read.vs));
    if (rc != FRR_OK) return rc;
    {
        // frr_draw on a partitioned ctx keeps only the triangles that touch the rank's tile rows of ITS window; that
        // list serves no other window or partition (the reference may reuse one geometry for several ranges,
        // renderer.rs:269-271: use frr_geometry for that, it never filters)
        const GeomPass &gp = f.geom;
        if (gp.read.filter && (gp.read.fy0 != y0 || gp.read.fy1 != y1 || gp.part_rank != f.bound.rank || gp.part_world != f.bound.world || gp.part_blocked != f.bound.part_blocked))
            return fail(c, FRR_ERR_INVALID, "the setup list was filtered by frr_draw for another window/partition; re-run frr_geometry (unfiltered) before frr_raster");
    }
    *nothing = x0 == x1 || y0 == y1 || f.geom.read.ntris == 0;
    return FRR_OK;
}

int frr_raster(frr_ctx *c, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1)
{
    if (!c) return FRR_ERR_INVALID;
    bool nothing = false;
    const int rc = raster_check(c, ps_id, x0, x1, y0, y1, &nothing);
    if (rc != FRR_OK || nothing) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    Cmd cmd = new_cmd(c, Cmd::RASTER, x0, x1, y0, y1);
    cmd.ps = ps_id; cmd.count_frags = c->count_frags;
    return exec_cmd(c, cmd);
}

// frr_draw*: the geometry pass `cmd`, then frr_raster of its setup list.  The raster window is known here, so a partitioned
// ctx can skip the setup records of triangles that touch none of its tile rows (frr_geometry* alone cannot: the window comes
// later).  raster: false for a list without items -- no vertex shader either, so nothing a pixel shader could fail to match
// (K_OF_NOTHING: the id has to name a shader, as frr_raster behind frr_geometry_list of it demands).
static int draw_pass(frr_ctx *c, Cmd &cmd, bool raster, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1)
{
    cmd.filter = c->fs.bound.world > 1 && y0 <= y1; cmd.fy0 = y0; cmd.fy1 = y1;
    const int rc = exec_cmd(c, cmd);
    if (rc != FRR_OK) return rc;
    if (!raster) return ps_check(c, K_OF_NOTHING, ps_id, 0);
    return frr_raster(c, ps_id, x0, x1, y0, y1);
}

int frr_draw(frr_ctx *c, int mesh, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1)
{
    if (!c || !slot_ok(c->meshes, mesh)) return fail(c, FRR_ERR_INVALID, "bad mesh id");
    HIP_TRY(c, hipSetDevice(c->device));
    Cmd cmd = new_cmd(c, Cmd::GEOM);
    cmd.mesh = mesh;
    return draw_pass(c, cmd, true, ps_id, x0, x1, y0, y1);
}

int frr_draw_instanced(frr_ctx *c, int mesh, int inst, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1)
{
    Cmd cmd;
    const int rc = instanced_cmd(c, mesh, inst, &cmd);
    return rc != FRR_OK ? rc : draw_pass(c, cmd, true, ps_id, x0, x1, y0, y1);
}

int frr_draw_list(frr_ctx *c, int list, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1)
{
    Cmd cmd;
    const int rc = list_cmd(c, list, &cmd);
    return rc != FRR_OK ? rc : draw_pass(c, cmd, c->lists[list].n != 0, ps_id, x0, x1, y0, y1);
}

int frr_draw_list_if(frr_ctx *c, int list, const void *dev_keep_u32, uint64_t keep_entries, uint32_t min_value, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1)
{
    Cmd cmd;
    const int rc = list_if_cmd(c, list, dev_keep_u32, keep_entries, min_value, &cmd);
    return rc != FRR_OK ? rc : draw_pass(c, cmd, c->lists[list].n != 0, ps_id, x0, x1, y0, y1);
}

int frr_frame_fence(frr_ctx *c, void *stream)
{
    if (!c) return FRR_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = settle(c); if (rc != FRR_OK) return rc; }
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (own_targets(c)) { c->exported[c->fs.bound.tset] = true; c->export_stream[c->fs.bound.tset] = st; }
    return fence_stream(c, st);
}

int frr_frame_wait(frr_ctx *c, void *stream)
{
    if (!c) return FRR_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    frr_ctx::FrameWait *w = nullptr;
    for (frr_ctx::FrameWait &p : c->waits) if (p.stream == st) w = &p;   // (the same stream again: the later record covers both)
    if (!w) {
        Event e;
        HIP_TRY(c, pooled_event(c->wait_pool, false, e));
        c->waits.push_back({st, std::move(e)});
        w = &c->waits.back();
    }
    HIP_TRY(c, hipEventRecord(w->ev, st));
    c->wait_serial += 1;
    return FRR_OK;
}

int frr_sync(frr_ctx *c)
{
    if (!c) return FRR_ERR_INVALID;
    const int rc = finish(c);
    c->sync_epoch += 1;   // the caller may rewrite a device-bound mesh in place now: its passes are verified again (DrawSig)
    return rc;
}

int frr_readback(frr_ctx *c, uint8_t *rgba, float *depth, uint32_t *tri_id)
{
    if (!c) return FRR_ERR_INVALID;
    { int rc = finish(c); if (rc != FRR_OK) return rc; }
    const size_t bytes = (size_t)c->W * c->H * 4;
    if (rgba) HIP_TRY(c, hipMemcpyAsync(rgba, c->fs.bound.color, bytes, hipMemcpyDeviceToHost, c->stream));
    if (depth) HIP_TRY(c, hipMemcpyAsync(depth, c->fs.bound.depth, bytes, hipMemcpyDeviceToHost, c->stream));
    if (tri_id) HIP_TRY(c, hipMemcpyAsync(tri_id, c->fs.bound.tri_id, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FRR_OK;
}

int frr_readback_setup(frr_ctx *c, frr_setup_vertex *out, uint64_t cap_tris, uint64_t *ntris)
{
    if (!c || !ntris || c->fs.geom.none()) return fail(c, FRR_ERR_INVALID, "no geometry to read back");
    { const int rc = need_unfiltered_list(c, "frr_readback_setup (the full Vec<[Vertex;3]>)"); if (rc != FRR_OK) return rc; }
    { int rcs = finish(c); if (rcs != FRR_OK) return rcs; }
    const FrameState &f = c->fs;
    const GeomTab &gt = c->hc.lane[f.lane].gtab[f.gpar()];
    const GeomSet &S = c->gset[f.geom.set];
    const uint64_t nt = f.geom.read.ntris;
    *ntris = nt ? gt.n_emit : 0;
    if (!out || !nt) return FRR_OK;
    // the records live at slots (frr_device.h): input t's own slot, or its fan's slots behind the inputs; walking the
    // inputs in order and each fan in order is the reference's emission order
    const uint64_t slots = nt + f.geom.fan_cap;   // (fan slots are spread over the regions of the fan space)
    const int K = frr_vs_num_varyings(f.geom.read.vs);
    std::vector<uint32_t> tinfo(nt), fanbase(nt);
    std::vector<RasterRec> recs(slots);
    std::vector<float> vary((size_t)slots * 3 * K);
    HIP_TRY(c, hipMemcpy(tinfo.data(), S.tinfo, nt * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(fanbase.data(), S.fanbase, nt * 4, hipMemcpyDeviceToHost));
    // the inputs' own slots, then the used part of every fan region
    const uint64_t region = f.geom.fan_cap / FAN_REGIONS;
    for (int k = -1; k < FAN_REGIONS; ++k) {
        const uint64_t first = k < 0 ? 0 : nt + (uint64_t)k * region;
        const uint64_t count = k < 0 ? nt : std::min<uint64_t>(gt.fan_cursor[k].v, region);
        if (!count) continue;
        HIP_TRY(c, hipMemcpy(recs.data() + first, S.recs + first, count * sizeof(RasterRec), hipMemcpyDeviceToHost));
        if (K) HIP_TRY(c, hipMemcpy(vary.data() + first * 3 * K, S.vary + first * 3 * K, count * 3 * K * sizeof(float), hipMemcpyDeviceToHost));
    }
    uint64_t i = 0;
    for (uint64_t t = 0; t < nt && i < cap_tris; ++t) {
        const uint32_t n = tinfo[t] & ((1u << FAN_BITS) - 1u);
        for (uint32_t q = 0; q < n && i < cap_tris; ++q, ++i) {
            const uint64_t slot = n == 1u ? t : nt + fanbase[t] + q;     // (a clipped input emits at least two triangles)
            if (slot >= slots) return fail(c, FRR_ERR_HIP, "setup tables are inconsistent");
            const RasterRec &r = recs[slot];
            const bool sw = r.flags & 1u;
            for (int v = 0; v < 3; ++v) {
                const int s = sw ? (v == 1 ? 2 : (v == 2 ? 1 : 0)) : v; // undo the orientation swap
                frr_setup_vertex &o = out[i * 3 + v];
                memset(&o, 0, sizeof o);
                o.spf[0] = r.s[2 * s]; o.spf[1] = r.s[2 * s + 1];
                o.spi[0] = spi_of(r.s[2 * s]); o.spi[1] = spi_of(r.s[2 * s + 1]);
                o.rhw = r.rhw[s];
                for (int k = 0; k < K; ++k) o.ctx[k] = vary[(size_t)slot * 3 * K + (size_t)s * K + k];
            }
        }
    }
    return FRR_OK;
}

// argument checks of frr_resolve_varyings / frr_readback_varyings; *K: varyings per vertex, *nothing: valid, writes nothing
static int vary_check(frr_ctx *c, int32_t x0, int32_t x1, int32_t y0, int32_t y1, const void *buf, uint64_t out_entries, int *K, bool *nothing)
{
    if (!c) return FRR_ERR_INVALID;
    const FrameState &f = c->fs;
    if (f.geom.none()) return fail(c, FRR_ERR_INVALID, "frr_resolve_varyings before frr_geometry");
    int rc = rule_rc(c, window_rule(WINDOW_ENTRIES, c->W, c->H, x0, x1, y0, y1));
    if (rc == FRR_OK) rc = need_unfiltered_list(c, "frr_resolve_varyings");
    if (rc == FRR_OK) rc = rule_rc(c, buffer_rule(BUFFER_VARYINGS_OUT, buf, out_entries, 0, x1, y0, y1));
    if (rc != FRR_OK) return rc;
    *K = frr_vs_num_varyings(f.geom.read.vs);
    *nothing = *K <= 0 || f.geom.read.ntris == 0;   // (geom.read.ntris == 0: an empty mesh, or frr_clear since -- the setup list is gone)
    return FRR_OK;
}

int frr_geometry_num_varyings(const frr_ctx *c)
{
    if (!c || c->fs.geom.none()) return FRR_ERR_INVALID;
    return frr_vs_num_varyings(c->fs.geom.read.vs);
}

int frr_resolve_varyings(frr_ctx *c, int32_t x0, int32_t x1, int32_t y0, int32_t y1, void *dev_out_f32, uint64_t out_entries)
{
    int K = 0; bool nothing = false;
    const int rc = vary_check(c, x0, x1, y0, y1, dev_out_f32, out_entries, &K, &nothing);
    if (rc != FRR_OK || nothing) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    Cmd cmd = new_cmd(c, Cmd::VARY, x0, x1, y0, y1);
    cmd.vary_out = (float *)dev_out_f32;
    return exec_cmd(c, cmd);
}

int frr_readback_varyings(frr_ctx *c, int32_t x0, int32_t x1, int32_t y0, int32_t y1, float *host_inout, uint64_t out_entries)
{
    int K = 0; bool nothing = false;
    const int rc = vary_check(c, x0, x1, y0, y1, host_inout, out_entries, &K, &nothing);
    if (rc != FRR_OK || nothing) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    // a temporary device buffer that starts as the caller's: what the command leaves untouched comes back as it went in
    const uint64_t entries = (uint64_t)((int64_t)y1 - y0) * (uint64_t)x1;
    const size_t bytes = (size_t)entries * (size_t)K * sizeof(float);
    DevBuf<float> tmp;
    if (tmp.reset((size_t)entries * (size_t)K) != hipSuccess) return nomem(c, "varyings buffer");
    const hipError_t e = hipMemcpy(tmp, host_inout, bytes, hipMemcpyHostToDevice);   // (returns when the copy is done: in front of the command on any stream)
    if (e != hipSuccess) return fail(c, FRR_ERR_HIP, std::string("hipMemcpy varyings: ") + hipGetErrorString(e));
    return host_round_trip(c, new_cmd(c, Cmd::VARY, x0, x1, y0, y1), &Cmd::vary_out, tmp, host_inout, bytes, "varyings");
}

// The count commands, frr_visible_pixels* and (`query`) frr_query_pixels*: the argument checks, the command, and with
// `host` its round trip through a temporary device buffer, after which *nunits is the number of units the pass has.
static int count_pixels(frr_ctx *c, bool query, bool host, int unit, int32_t x0, int32_t x1, int32_t y0, int32_t y1, void *out, uint64_t out_entries, uint64_t *nunits)
{
    if (!c) return FRR_ERR_INVALID;
    const char *who = query ? "frr_query_pixels" : "frr_visible_pixels";
    const FrameState &f = c->fs;
    if (unit != FRR_PER_ITEM && unit != FRR_PER_TRIANGLE) return fail(c, FRR_ERR_INVALID, "unknown frr_visible_unit");
    if (f.geom.none()) return fail(c, FRR_ERR_INVALID, std::string(who) + " before any geometry pass");
    int rc = rule_rc(c, window_rule(WINDOW_ENTRIES, c->W, c->H, x0, x1, y0, y1));
    if (rc == FRR_OK) rc = need_unfiltered_list(c, who);
    if (rc == FRR_OK) rc = rule_rc(c, buffer_rule(BUFFER_COUNTS_OUT, out, out_entries, 0, x1, y0, y1));
    const uint32_t *item_first;   // (a query over a list freed since the pass: refused here, before anything is launched)
    if (rc == FRR_OK && query && unit == FRR_PER_ITEM && f.draws != 0) rc = list_item_first(c, &item_first);
    if (rc != FRR_OK || out_entries == 0) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    // a query is a raster command that counts, or -- a frr_clear since the pass, a pass without triangles or without items:
    // nothing to rasterize -- the count command, which then zeroes the buffer and counts nothing
    const bool raster = query && f.draws != 0 && f.geom.read.ntris != 0 && !(unit == FRR_PER_ITEM && f.geom.nitems == 0);
    Cmd cmd = new_cmd(c, raster ? Cmd::RASTER : Cmd::VISIBLE, x0, x1, y0, y1);
    if (query) { cmd.query = true; cmd.ps = FRR_PS_DEPTH; cmd.count_frags = false; }
    cmd.vis_unit = unit; cmd.vis_out = host ? nullptr : (uint32_t *)out; cmd.vis_entries = out_entries;
    if (!host) return exec_cmd(c, cmd);
    DevBuf<uint32_t> tmp;
    if (tmp.reset((size_t)out_entries) != hipSuccess) return nomem(c, "count buffer");
    rc = host_round_trip(c, cmd, &Cmd::vis_out, tmp, (uint32_t *)out, (size_t)out_entries * sizeof(uint32_t), "counts");
    if (rc != FRR_OK) return rc;
    if (nunits) {
        const GeomTab &gt = c->hc.lane[f.lane].gtab[f.gpar()];
        *nunits = unit == FRR_PER_ITEM ? f.geom.nitems : f.draws == 0 ? 0 : (uint64_t)gt.tri_base + (f.geom.read.ntris ? gt.n_emit : 0u);
    }
    return FRR_OK;
}

int frr_visible_pixels(frr_ctx *c, int unit, int32_t x0, int32_t x1, int32_t y0, int32_t y1, void *dev_out_u32, uint64_t out_entries)
{
    return count_pixels(c, false, false, unit, x0, x1, y0, y1, dev_out_u32, out_entries, nullptr);
}
int frr_visible_pixels_host(frr_ctx *c, int unit, int32_t x0, int32_t x1, int32_t y0, int32_t y1, uint32_t *host_out, uint64_t out_entries, uint64_t *nunits)
{
    return count_pixels(c, false, true, unit, x0, x1, y0, y1, host_out, out_entries, nunits);
}
int frr_query_pixels(frr_ctx *c, int unit, int32_t x0, int32_t x1, int32_t y0, int32_t y1, void *dev_out_u32, uint64_t out_entries)
{
    return count_pixels(c, true, false, unit, x0, x1, y0, y1, dev_out_u32, out_entries, nullptr);
}
int frr_query_pixels_host(frr_ctx *c, int unit, int32_t x0, int32_t x1, int32_t y0, int32_t y1, uint32_t *host_out, uint64_t out_entries, uint64_t *nunits)
{
    return count_pixels(c, true, true, unit, x0, x1, y0, y1, host_out, out_entries, nunits);
}

int frr_host_fragment_passes(float rhw, float depth) { return fragment_passes(rhw, depth) ? 1 : 0; }

// ---- box queries (frr_boxes.h) -----------------------------------------------------------------------------------------
int frr_drawlist_bounds(frr_ctx *c, int list, float *host_lo_hi, uint32_t *host_flags, uint64_t cap, uint64_t *nitems)
{
    if (!c || !slot_ok(c->lists, list)) return fail(c, FRR_ERR_INVALID, "bad draw list id");
    if (c->lists[list].dead) return fail(c, FRR_ERR_INVALID, "a mesh the draw list names was freed: the list is dead (frr_drawlist_free still takes it)");
    const uint64_t n = c->lists[list].n;
    int rc = n ? rule_rc(c, bounds_rule(c->lists[list].vs)) : FRR_OK;
    if (rc != FRR_OK) return rc;
    // a table of this list may be read by a command in flight or in the log: nothing reads it any more after this
    if ((rc = finish(c)) != FRR_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    DrawList &dl = c->lists[list];
    dl.has_bounds = false;
    if (nitems) *nitems = n;
    if (n == 0) { dl.has_bounds = true; return FRR_OK; }
    // the distinct meshes of the snapshot: one reduction each
    const uint32_t nf = (uint32_t)frr_vs_input_floats(dl.vs);
    std::vector<BoundsJob> jobs;
    std::vector<uint32_t> item_job(n), keys;
    std::map<std::pair<const void *, std::pair<const void *, uint64_t>>, uint32_t> seen;
    uint32_t most = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const ListRow &r = dl.hrows[i];
        const auto key = std::make_pair((const void *)r.verts, std::make_pair((const void *)r.idx, ((uint64_t)r.nverts << 32) | r.ntris));
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (uint32_t)jobs.size()).first;
            jobs.push_back(BoundsJob{r.verts, r.idx, r.nverts, r.ntris, nf, 0u});
            most = std::max(most, r.ntris);
        }
        item_job[i] = it->second;
    }
    keys.resize(jobs.size() * 8);
    for (size_t j = 0; j < jobs.size(); ++j) for (int k = 0; k < 8; ++k) keys[8 * j + k] = k < 3 ? 0xFFFFFFFFu : 0u;
    DevBuf<BoundsJob> djobs; DevBuf<uint32_t> ditem, dkeys; DevBuf<float> lo_hi; DevBuf<uint32_t> flags;
    if (lo_hi.reset((size_t)n * 6) != hipSuccess || flags.reset((size_t)n) != hipSuccess) return nomem(c, "bounds table");
    if ((rc = upload(c, djobs, jobs.data(), jobs.size() * sizeof(BoundsJob), "bounds jobs", false)) != FRR_OK) return rc;
    if ((rc = upload(c, ditem, item_job.data(), item_job.size() * sizeof(uint32_t), "bounds jobs", false)) != FRR_OK) return rc;
    if ((rc = upload(c, dkeys, keys.data(), keys.size() * sizeof(uint32_t), "bounds jobs", false)) != FRR_OK) return rc;
    // on the ctx's stream, behind what the caller has put there (a device-bound mesh's vertices), as k_index_check runs
    {
        ProfScope p(c, KID_BOXES, c->stream);
        const uint32_t chunks = std::min<uint32_t>((most + BOX_WG_TRIS - 1) / BOX_WG_TRIS, c->box_bounds_chunks ? c->box_bounds_chunks : 1024u);
        if (chunks) hipLaunchKernelGGL(k_box_bounds, dim3(chunks, (uint32_t)jobs.size()), dim3(BOX_WG), 0, c->stream, djobs.get(), dkeys.get());
        hipLaunchKernelGGL(k_box_bounds_finish, dim3((uint32_t)((n + BOX_WG - 1) / BOX_WG)), dim3(BOX_WG), 0, c->stream, dkeys.get(), ditem.get(), djobs.get(), (uint32_t)n, lo_hi.get(), flags.get());
    }
    hipError_t e = hipGetLastError();
    const uint64_t take = std::min<uint64_t>(cap, n);
    if (e == hipSuccess && host_lo_hi && take) e = hipMemcpyAsync(host_lo_hi, lo_hi.get(), (size_t)take * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && host_flags && take) e = hipMemcpyAsync(host_flags, flags.get(), (size_t)take * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_rc(c, e);
    dl.box_lo_hi = std::move(lo_hi); dl.box_flags = std::move(flags); dl.has_bounds = true;
    return FRR_OK;
}

// frr_query_boxes*: the argument checks, the command, and with `host` its round trip through a temporary device buffer
static int query_boxes(frr_ctx *c, bool host, int list, int32_t x0, int32_t x1, int32_t y0, int32_t y1, void *out, uint64_t out_entries, uint64_t *nunits)
{
    if (!c || !slot_ok(c->lists, list)) return fail(c, FRR_ERR_INVALID, "bad draw list id");
    const DrawList &dl = c->lists[list];
    if (dl.dead) return fail(c, FRR_ERR_INVALID, "a mesh the draw list names was freed: the list is dead (frr_drawlist_free still takes it)");
    int rc = rule_rc(c, boxes_rule(dl.has_bounds));
    if (rc == FRR_OK) rc = rule_rc(c, window_rule(WINDOW_ENTRIES, c->W, c->H, x0, x1, y0, y1));
    if (rc == FRR_OK) rc = rule_rc(c, buffer_rule(BUFFER_COUNTS_OUT, out, out_entries, 0, x1, y0, y1));
    if (rc != FRR_OK || out_entries == 0) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    Cmd cmd = new_cmd(c, Cmd::BOXES, x0, x1, y0, y1);
    cmd.list = list; cmd.list_gen = dl.gen;
    h_mat4_mul(c->uni.proj, c->uni.view, cmd.pv);   // as list_cmd takes it: the list pass's mvp = pv * model
    cmd.vis_out = host ? nullptr : (uint32_t *)out; cmd.vis_entries = out_entries;
    if (!host) return exec_cmd(c, cmd);
    DevBuf<uint32_t> tmp;
    if (tmp.reset((size_t)out_entries) != hipSuccess) return nomem(c, "count buffer");
    rc = host_round_trip(c, cmd, &Cmd::vis_out, tmp, (uint32_t *)out, (size_t)out_entries * sizeof(uint32_t), "box counts");
    if (rc == FRR_OK && nunits) *nunits = c->lists[list].n;
    return rc;
}
int frr_query_boxes(frr_ctx *c, int list, int32_t x0, int32_t x1, int32_t y0, int32_t y1, void *dev_out_u32, uint64_t out_entries)
{
    return query_boxes(c, false, list, x0, x1, y0, y1, dev_out_u32, out_entries, nullptr);
}
int frr_query_boxes_host(frr_ctx *c, int list, int32_t x0, int32_t x1, int32_t y0, int32_t y1, uint32_t *host_out, uint64_t out_entries, uint64_t *nunits)
{
    return query_boxes(c, true, list, x0, x1, y0, y1, host_out, out_entries, nunits);
}
int64_t frr_host_query_boxes(const float *mvps, const float *lo_hi, const uint32_t *flags, uint64_t nitems, uint32_t W, uint32_t H,
                             int32_t x0, int32_t x1, int32_t y0, int32_t y1, const float *depth, uint64_t depth_entries, const uint8_t *row_owned,
                             uint32_t *out, uint64_t out_entries, int32_t *status_rect_level)
{
    if ((nitems && (!mvps || !lo_hi || !flags)) || !depth || (out_entries && !out)) return -1;
    if (window_rule(WINDOW_ENTRIES, W, H, x0, x1, y0, y1).code != FRR_OK) return -1;
    if ((uint64_t)((int64_t)y1 - y0 - 1) * (uint64_t)x1 + (uint64_t)((int64_t)x1 - x0) > depth_entries) return -1;   // the last entry the window reads
    return box_host_query(mvps, lo_hi, flags, nitems, BoxWindow{W, H, x0, x1, y0, y1}, depth, row_owned, out, out_entries, status_rect_level);
}

int64_t frr_host_visible_counts(const uint32_t *ids, uint64_t id_entries, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                                const uint32_t *bounds, uint64_t nunits, uint32_t *out, uint64_t out_entries)
{
    if (!ids || (out_entries && !out) || x0 < 0 || x1 <= x0 || y1 <= y0 || nunits > 0xFFFFFFFFull) return -1;
    if ((uint64_t)((int64_t)y1 - y0 - 1) * (uint64_t)x1 + (uint64_t)((int64_t)x1 - x0) > id_entries) return -1;   // the last entry the window reads
    if (bounds) for (uint64_t k = 0; k < nunits; ++k) if (bounds[k] > bounds[k + 1]) return -1;
    return (int64_t)visible_counts_host(ids, x0, x1, y0, y1, bounds, nunits, out, out_entries);
}

// argument checks of frr_shade_varyings / frr_shade_varyings_host; *nothing: the call is valid and writes nothing
static int shade_check(frr_ctx *c, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1, const void *buf, uint64_t in_entries, int K, uint32_t id_count, bool *nothing)
{
    if (!c) return FRR_ERR_INVALID;
    int rc = rule_rc(c, window_rule(WINDOW_ENTRIES, c->W, c->H, x0, x1, y0, y1));
    if (rc == FRR_OK) rc = ps_check(c, K_OF_BUFFER, ps_id, K);   // the rule frr_raster applies, with the buffer's K for the geometry's
    if (rc == FRR_OK) rc = rule_rc(c, buffer_rule(BUFFER_VARYINGS_IN, buf, in_entries, K, x1, y0, y1));
    *nothing = id_count == 0u;
    return rc;
}
static Cmd shade_cmd(const frr_ctx *c, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1, const float *dev_in, uint64_t in_entries, int K, uint32_t id_first, uint32_t id_count)
{
    Cmd cmd = new_cmd(c, Cmd::SHADE, x0, x1, y0, y1);
    cmd.ps = ps_id; cmd.shade_in = dev_in; cmd.shade_entries = in_entries; cmd.shade_K = K; cmd.id_first = id_first; cmd.id_count = id_count;
    return cmd;
}

int frr_shade_varyings(frr_ctx *c, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1, const void *dev_in_f32, uint64_t in_entries, int K,
                       uint32_t id_first, uint32_t id_count)
{
    bool nothing = false;
    const int rc = shade_check(c, ps_id, x0, x1, y0, y1, dev_in_f32, in_entries, K, id_count, &nothing);
    if (rc != FRR_OK || nothing) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return exec_cmd(c, shade_cmd(c, ps_id, x0, x1, y0, y1, (const float *)dev_in_f32, in_entries, K, id_first, id_count));
}

int frr_shade_varyings_host(frr_ctx *c, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1, const float *host_in, uint64_t in_entries, int K,
                            uint32_t id_first, uint32_t id_count)
{
    bool nothing = false;
    const int rc = shade_check(c, ps_id, x0, x1, y0, y1, host_in, in_entries, K, id_count, &nothing);
    if (rc != FRR_OK || nothing) return rc;
    return shade_from_host(c, shade_cmd(c, ps_id, x0, x1, y0, y1, nullptr, 0, K, id_first, id_count), host_in);
}

// ---- per-item materials (frr_shade_items): tables of frr_material, one entry per item of a pass ----------------------
static int bad_material(frr_ctx *c, uint64_t k)
{
    return fail(c, FRR_ERR_INVALID, "materials: entry " + std::to_string(k) + " has a texture_slot outside 0 .. " + std::to_string(FRR_MAX_TEXTURES - 1) + " or reserved != 0");
}
static int materials_register(frr_ctx *c, Materials &&t, uint64_t n, uint32_t slots, int *materials_out)
{
    if (t.own) t.dev = t.own;
    t.n = n; t.slots = slots; t.used = true;
    *materials_out = slot_put(c->materials, std::move(t));
    return FRR_OK;
}
int frr_materials_upload(frr_ctx *c, const frr_material *mats, uint64_t n, int *materials_out)
{
    if (!c || !materials_out) return fail(c, FRR_ERR_INVALID, "bad material table");
    { const int rc = rule_rc(c, materials_rule(MATERIALS_UPLOAD, mats, n)); if (rc != FRR_OK) return rc; }
    uint32_t slots = 0;
    for (uint64_t k = 0; k < n; ++k) {
        if (!material_ok(mats[k])) return bad_material(c, k);
        slots |= 1u << mats[k].texture_slot;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    Materials t;
    if (n) { const int rc = upload(c, t.own, mats, (size_t)n * sizeof(frr_material), "material table"); if (rc != FRR_OK) return rc; }
    return materials_register(c, std::move(t), n, slots, materials_out);
}
int frr_materials_bind_device(frr_ctx *c, const void *dev_mats, uint64_t n, int *materials_out)
{
    if (!c || !materials_out) return fail(c, FRR_ERR_INVALID, "bad material table");
    { const int rc = rule_rc(c, materials_rule(MATERIALS_BIND, dev_mats, n)); if (rc != FRR_OK) return rc; }
    if (n > 0xFFFFFFFFull) return fail(c, FRR_ERR_UNSUPPORTED, "2^32 materials or more");
    uint32_t cell_h[2] = {0xFFFFFFFFu, 0u};   // the first bad entry, the slots the table names
    if (n) {   // one reduction on the caller's stream -- behind whatever wrote the table -- and the host waits for it (a set-up call)
        HIP_TRY(c, hipSetDevice(c->device));
        DevBuf<uint32_t> cell;
        if (cell.reset(2) != hipSuccess) return nomem(c, "check cell");
        hipError_t e = hipMemcpyAsync(cell.get(), cell_h, sizeof cell_h, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_materials_check, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 1024)), dim3(256), 0, c->stream, (const frr_material *)dev_mats, (uint32_t)n, cell.get());
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(cell_h, cell.get(), sizeof cell_h, hipMemcpyDeviceToHost, c->stream);
        { const int rc = hip_rc(c, e == hipSuccess ? hipStreamSynchronize(c->stream) : e); if (rc != FRR_OK) return rc; }
        if (cell_h[0] != 0xFFFFFFFFu) return bad_material(c, cell_h[0]);
    }
    Materials t; t.dev = (const frr_material *)dev_mats;
    return materials_register(c, std::move(t), n, cell_h[1], materials_out);   // (the host wait above stands for a join of the ctx's private streams)
}
int frr_materials_free(frr_ctx *c, int materials)
{
    if (!c || !slot_ok(c->materials, materials)) return fail(c, FRR_ERR_INVALID, "bad material table id");
    { int rc = finish(c); if (rc != FRR_OK) return rc; }   // nothing reads it any more, nothing will replay a shade over it
    c->materials[materials] = Materials();
    return FRR_OK;
}

// argument checks of frr_shade_items / frr_shade_items_host; *nothing: the call is valid and writes nothing
static int shade_items_check(frr_ctx *c, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1, const void *buf, uint64_t in_entries, int K, int materials, bool *nothing)
{
    if (!c) return FRR_ERR_INVALID;
    int rc = rule_rc(c, window_rule(WINDOW_ENTRIES, c->W, c->H, x0, x1, y0, y1));
    if (rc == FRR_OK) {   // (the texture of a lit shader is the materials' business: below)
        const UserShader *us = ps_id >= FRR_SHADER_USER_BASE ? user_shader(ps_id) : nullptr;
        rc = rule_rc(c, pixel_shader_rule(K_OF_BUFFER, ps_id, K, us ? us->K : USER_K_UNKNOWN, true));
    }
    if (rc == FRR_OK) rc = rule_rc(c, buffer_rule(BUFFER_VARYINGS_IN, buf, in_entries, K, x1, y0, y1));
    if (rc != FRR_OK) return rc;
    if (!slot_ok(c->materials, materials)) return fail(c, FRR_ERR_INVALID, "bad material table id");
    const FrameState &f = c->fs;
    if (f.geom.none()) return fail(c, FRR_ERR_INVALID, "frr_shade_items before any geometry pass");
    if ((rc = need_unfiltered_list(c, "frr_shade_items")) != FRR_OK) return rc;
    const Materials &M = c->materials[materials];
    uint32_t filled = 0;
    for (int s = 0; s < FRR_MAX_TEXTURES; ++s) if (c->tex[s].dev) filled |= 1u << s;
    int which = -1;
    const Rule r = materials_rule(MATERIALS_SHADE, M.dev, M.n, f.geom.nitems, ps_id == FRR_PS_PHONG || ps_id == FRR_PS_BLINN, M.slots, filled, &which);
    if (r.code != FRR_OK) return fail(c, r.code, which >= 0 ? std::string(r.msg) + ": slot " + std::to_string(which) : std::string(r.msg));
    // frr_clear since the pass (the id target holds nothing of it, its tables are gone), a pass without inputs, no items
    *nothing = f.draws == 0 || f.geom.read.ntris == 0 || f.geom.nitems == 0;
    return FRR_OK;
}
static Cmd shade_items_cmd(const frr_ctx *c, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1, const float *dev_in, uint64_t in_entries, int K, int materials)
{
    Cmd cmd = new_cmd(c, Cmd::SHADE_ITEMS, x0, x1, y0, y1);
    cmd.ps = ps_id; cmd.shade_in = dev_in; cmd.shade_entries = in_entries; cmd.shade_K = K;
    cmd.mats = c->materials[materials].dev;
    return cmd;
}

int frr_shade_items(frr_ctx *c, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1, const void *dev_in_f32, uint64_t in_entries, int K, int materials)
{
    bool nothing = false;
    const int rc = shade_items_check(c, ps_id, x0, x1, y0, y1, dev_in_f32, in_entries, K, materials, &nothing);
    if (rc != FRR_OK || nothing) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return exec_cmd(c, shade_items_cmd(c, ps_id, x0, x1, y0, y1, (const float *)dev_in_f32, in_entries, K, materials));
}

int frr_shade_items_host(frr_ctx *c, int ps_id, int32_t x0, int32_t x1, int32_t y0, int32_t y1, const float *host_in, uint64_t in_entries, int K, int materials)
{
    bool nothing = false;
    const int rc = shade_items_check(c, ps_id, x0, x1, y0, y1, host_in, in_entries, K, materials, &nothing);
    if (rc != FRR_OK || nothing) return rc;
    return shade_from_host(c, shade_items_cmd(c, ps_id, x0, x1, y0, y1, nullptr, 0, K, materials), host_in);
}

int64_t frr_host_entry_items(const uint32_t *ids, uint64_t id_entries, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                             const uint32_t *bounds, uint64_t nitems, uint32_t *item_out)
{
    if (!ids || !item_out || !bounds || x0 < 0 || x1 <= x0 || y1 <= y0 || nitems >= 0xFFFFFFFFull) return -1;
    if ((uint64_t)((int64_t)y1 - y0 - 1) * (uint64_t)x1 + (uint64_t)((int64_t)x1 - x0) > id_entries) return -1;   // the last entry the window reads
    for (uint64_t k = 0; k < nitems; ++k) if (bounds[k] > bounds[k + 1]) return -1;
    if (nitems == 0) {
        for (int64_t ry = 0; ry < (int64_t)y1 - y0; ++ry) for (int64_t cx = 0; cx < (int64_t)x1 - x0; ++cx) item_out[(uint64_t)ry * (uint64_t)x1 + (uint64_t)cx] = VIS_NONE;
        return 0;
    }
    return (int64_t)entry_items_host(ids, x0, x1, y0, y1, bounds, (uint32_t)nitems, item_out);
}

int frr_get_stats(frr_ctx *c, frr_stats *out)
{
    if (!c || !out) return FRR_ERR_INVALID;
    { int rc = finish(c); if (rc != FRR_OK) return rc; }
    const FrameState &f = c->fs;
    const Lane &h = c->hc.lane[f.lane];
    const bool tot = h.totals_frame == f.frame_no;
    memset(out, 0, sizeof *out);
    out->tris_in = f.tris_in;
    out->draws = f.draws;
    out->replays = c->replays;
    out->frag_covered = tot ? h.tot_frag_covered : 0;
    out->frag_nan = tot ? h.tot_frag_nan : 0;
    out->bin_entries = tot ? h.tot_bin_entries : 0;
    for (int p = 0; p < 2; ++p) {
        if (h.gtab[p].frame_no == f.frame_no) { out->frag_covered += h.gtab[p].frag_covered; out->frag_nan += h.gtab[p].frag_nan; }
        if (h.btab[p].frame_no == f.frame_no) out->bin_entries += h.btab[p].seg_total;
    }
    if (f.draws && h.gtab[f.gpar()].frame_no == f.frame_no) out->tris_setup = (uint64_t)h.gtab[f.gpar()].tri_base + h.gtab[f.gpar()].n_emit;
#ifdef FRR_DEBUG_COUNTERS
    if (getenv("FRR_DEBUG_PRINT")) {
        fprintf(stderr, "frr dbg:");
        for (int k = 0; k < 24; ++k) {
            unsigned long long v = 0;
            for (int j = 0; j < DBG_COPIES; ++j) v += c->hc.dbg[j][k];
            fprintf(stderr, " %llu", v);
        }
        fprintf(stderr, "\n");
    }
#endif
    return FRR_OK;
}

int frr_event_record(frr_ctx *c, int slot)
{
    if (!c || slot < 0 || slot >= 16) return FRR_ERR_INVALID;
    // (a measuring call: the caller's stream first waits for the ctx's other streams, so that the event brackets whole frames)
    if (c->g_used) { HIP_TRY(c, hipEventRecord(c->ev_join, c->gstream)); HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0)); }
    { int rcj = join_tile_streams(c); if (rcj != FRR_OK) return rcj; }
    HIP_TRY(c, hipEventRecord(c->ev[slot], c->stream));
    c->ev_set[slot] = true;
    return FRR_OK;
}
int frr_event_elapsed_ms(frr_ctx *c, int a, int b, float *ms)
{
    if (!c || !ms || a < 0 || a >= 16 || b < 0 || b >= 16 || !c->ev_set[a] || !c->ev_set[b]) return FRR_ERR_INVALID;
    HIP_TRY(c, hipEventSynchronize(c->ev[b]));
    HIP_TRY(c, hipEventElapsedTime(ms, c->ev[a], c->ev[b]));
    return FRR_OK;
}
int frr_profile_enable(frr_ctx *c, int enable)
{
    if (!c) return FRR_ERR_INVALID;
    prof_collect(c);
    c->prof_mask = enable < 0 ? 0xFFFFFFFFu : (uint32_t)enable;
    return FRR_OK;
}
int frr_tile_order_passes(frr_ctx *c, uint64_t *passes)
{
    if (!c || !passes) return FRR_ERR_INVALID;
    *passes = c->ordered_passes;
    return FRR_OK;
}
int frr_profile_set_period(frr_ctx *c, uint32_t period)
{
    if (!c || period == 0) return FRR_ERR_INVALID;
    c->prof_period = period;
    for (int i = 0; i < KID_COUNT; ++i) c->prof_seen[i] = 0;
    return FRR_OK;
}
int frr_profile_reset(frr_ctx *c)
{
    if (!c) return FRR_ERR_INVALID;
    prof_collect(c);
    for (int i = 0; i < KID_COUNT; ++i) { c->prof_ms[i] = 0; c->prof_n[i] = 0; }
    return FRR_OK;
}
int frr_profile_get(frr_ctx *c, const char *kernel, float *total_ms, uint32_t *launches)
{
    if (!c || !kernel) return FRR_ERR_INVALID;
    prof_collect(c);
    for (int i = 0; i < KID_COUNT; ++i)
        if (strcmp(kernel, kKernelNames[i]) == 0) {
            if (total_ms) *total_ms = (float)c->prof_ms[i];
            if (launches) *launches = c->prof_n[i];
            return FRR_OK;
        }
    return FRR_ERR_INVALID;
}

// ---- host helpers: matrix_util.rs:3-35 ------------------------------------------------------
void frr_set_identity(float m[16])
{
    for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}
static inline float h_dot3(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static inline void h_norm3(float *v) { float r = 1.0f / sqrtf(h_dot3(v, v)); v[0] *= r; v[1] *= r; v[2] *= r; }
static inline void h_cross3(const float *a, const float *b, float *o)
{
    o[0] = a[1] * b[2] - b[1] * a[2]; o[1] = a[2] * b[0] - b[2] * a[0]; o[2] = a[0] * b[1] - b[0] * a[1];
}
void frr_set_look_at(const float eye[3], const float at[3], const float up[3], float m[16])
{
    float z[3] = {at[0] - eye[0], at[1] - eye[1], at[2] - eye[2]}, x[3], y[3];
    h_norm3(z);                 // z_axis = (at - eye).normalize()      :11
    h_cross3(up, z, x); h_norm3(x); // x_axis = up.cross(z_axis).normalize() :12
    h_cross3(z, x, y);          // y_axis = z_axis.cross(x_axis)         :13
    m[0] = x[0]; m[1] = y[0]; m[2] = z[0]; m[3] = 0.0f;
    m[4] = x[1]; m[5] = y[1]; m[6] = z[1]; m[7] = 0.0f;
    m[8] = x[2]; m[9] = y[2]; m[10] = z[2]; m[11] = 0.0f;
    m[12] = -h_dot3(eye, x); m[13] = -h_dot3(eye, y); m[14] = -h_dot3(eye, z); m[15] = 1.0f;
}
void frr_set_perspective(float fovy, float aspect, float zn, float zf, float m[16])
{
    const float fax = 1.0f / tanf(fovy * 0.5f);         // f32::tan(..).recip()  :26
    memset(m, 0, 16 * sizeof(float));
    m[0] = fax / aspect;                                // :28
    m[5] = fax;                                         // :29
    m[10] = zf / (zf - zn);                             // :30
    m[14] = -zn * zf / (zf - zn);                       // :31
    m[11] = 1.0f;                                       // :32
}

// ---- debug hooks ------------------------------------------------------------------------------
float frr_host_atan2f(float y, float x) { return fd_atan2f(y, x); }
float frr_host_cull_det(const float clip[12])
{
    float pos[3][4];
    memcpy(pos, clip, sizeof pos);
    return cull_det(pos);
}

int frr_debug_mvp(frr_ctx *c, int mesh, int use_mfma, float *clip_out, float *ms_out)
{
    if (!c || !slot_ok(c->meshes, mesh) || !clip_out) return fail(c, FRR_ERR_INVALID, "bad arguments");
    const Mesh &m = c->meshes[mesh];
    if (m.vs != FRR_VS_PHONG && m.vs != FRR_VS_GOURAUD) return fail(c, FRR_ERR_INVALID, "needs a pos3/uv2/normal3 mesh");
    if (m.idx) return fail(c, FRR_ERR_UNSUPPORTED, "frr_debug_mvp reads an expanded mesh, not an indexed one");
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t nverts = (uint32_t)(m.ntris * 3);
    DevBuf<float4> d;
    if (d.reset((size_t)nverts + 1) != hipSuccess) return nomem(c, "debug buffer");
    const dim3 grid((nverts + 63) / 64), block(64);
    Event e0, e1; (void)e0.create(true); (void)e1.create(true);
    for (int it = 0; it < 3; ++it) { // last iteration is the timed one
        (void)hipEventRecord(e0, c->stream);
        if (use_mfma) hipLaunchKernelGGL(k_debug_mvp_mfma, grid, block, 0, c->stream, m.dev, nverts, 8, c->duni, d);
        else hipLaunchKernelGGL(k_debug_mvp_exact, grid, block, 0, c->stream, m.dev, nverts, 8, c->duni, d);
        (void)hipEventRecord(e1, c->stream);
    }
    hipError_t e = hipMemcpyAsync(clip_out, d, (size_t)nverts * 16, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (ms_out) *ms_out = ms;
    return hip_rc(c, e);
}

int frr_debug_gather_calib(frr_ctx *c, uint32_t log2_records)
{
    if (!c || log2_records < 10 || log2_records > 24) return FRR_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)1 << log2_records;
    DevBuf<uint4> d;   // n records of 64 bytes and the cell the kernel writes
    if (d.reset(n * 4 + 4) != hipSuccess) return nomem(c, "debug buffer");
    hipError_t e = hipMemsetAsync(d, 1, n * 64 + 64, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_debug_gather, dim3((uint32_t)(n / 256)), dim3(256), 0, c->stream, (const uint4 *)d.get(), (uint32_t)(n - 1), (uint32_t *)(d.get() + n * 4));
        e = hipStreamSynchronize(c->stream);
    }
    return hip_rc(c, e);
}

int frr_debug_rcp_check(frr_ctx *c, uint32_t lo_bits, uint32_t hi_bits, uint64_t *mismatches, uint32_t *first_bad)
{
    if (!c || !mismatches || !first_bad) return FRR_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<unsigned long long> d;
    if (d.reset(2) != hipSuccess) return nomem(c, "debug buffer");
    const unsigned long long init[2] = {0ull, 0xFFFFFFFFull};
    hipError_t e = hipMemcpyAsync(d, init, 16, hipMemcpyHostToDevice, c->stream);
    unsigned long long out[2] = {0, 0};
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_debug_rcp, dim3(4096), dim3(256), 0, c->stream, lo_bits, hi_bits, d.get(), (uint32_t *)(d + 1));
        e = hipMemcpyAsync(out, d, 16, hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, FRR_ERR_HIP, hipGetErrorString(e));
    *mismatches = out[0];
    *first_bad = (uint32_t)out[1];
    return FRR_OK;
}

#ifdef FRR_DEBUG_COUNTERS
// dev builds only (not part of include/frr.h): the per-tile timeline of the latest tile kernel, [max_tiles][8] u64
int frr_debug_tiles(frr_ctx *c, unsigned long long *out, uint32_t *ntiles)
{
    if (!c || !out || !ntiles || !c->dbg_tiles) return FRR_ERR_INVALID;
    { int rc = drain(c); if (rc != FRR_OK) return rc; }
    HIP_TRY(c, hipMemcpy(out, c->dbg_tiles, (size_t)c->max_tiles * 64, hipMemcpyDeviceToHost));
    *ntiles = c->max_tiles;
    return FRR_OK;
}
#endif

int frr_debug_scan64(frr_ctx *c, const uint32_t *in, uint32_t *out)
{
    if (!c || !in || !out) return FRR_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<uint32_t> d;
    if (d.reset(128) != hipSuccess) return nomem(c, "debug buffer");
    hipError_t e = hipMemcpyAsync(d, in, 64 * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_debug_scan, dim3(1), dim3(64), 0, c->stream, d.get(), d + 64);
        e = hipMemcpyAsync(out, d + 64, 64 * 4, hipMemcpyDeviceToHost, c->stream);
    }
    return hip_rc(c, e == hipSuccess ? hipStreamSynchronize(c->stream) : e);
}

int frr_debug_atan2f(frr_ctx *c, const float *y, const float *x, float *out, uint64_t n)
{
    if (!c || !y || !x || !out) return FRR_ERR_INVALID;
    if (n == 0) return FRR_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float> d;
    if (d.reset(n * 3) != hipSuccess) return nomem(c, "debug buffer");
    hipError_t e = hipMemcpyAsync(d, y, n * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + n, x, n * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_debug_atan2f, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, d.get(), d + n, d + 2 * n, n);
        e = hipMemcpyAsync(out, d + 2 * n, n * 4, hipMemcpyDeviceToHost, c->stream);
    }
    return hip_rc(c, e == hipSuccess ? hipStreamSynchronize(c->stream) : e);
}

} // extern "C"
