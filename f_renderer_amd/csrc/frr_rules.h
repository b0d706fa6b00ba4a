// frr_rules.h -- the argument rules of the commands (frr_api.hip), each stated once: which window, which pixel shader and
// which buffer a call may name, and the most inputs a geometry pass takes.  Plain C++ (no HIP), so that a CPU test can hold
// the rules, beside a port of the reference where they stand for something it does (tests/test_arg_rules_cpu.py).
//
// What the rules stand for in the reference.  Renderer::rasterization clamps every triangle's bounding box into the
// caller's ranges -- i32::clamp(min, max) panics where min > max (renderer.rs:285) -- and addresses the depth buffer at
// (cy - y0) * x1 + (cx - x0) (renderer.rs:362), which panics where that index leaves the buffer: a window the library
// refuses with FRR_ERR_INVALID is one the reference would not have survived, or one this library has no buffer for (it is
// stricter than the reference: it refuses by the window alone, the reference only where a triangle gets there).  The two
// closures of a draw share one ShaderContext type (renderer.rs:97-110): a pixel shader reads the varyings its vertex
// shader wrote, so the two have to agree on their number K.  FRR_ERR_UNSUPPORTED is a limit of this library alone.
//
// A rule answers with a status code of include/frr.h and a static text; what needs a ctx (is there a geometry pass, was its
// setup list filtered, which K a user shader was registered with) is asked in frr_api.hip, in the order each entry point
// has always asked.
#pragma once
#include <stdint.h>
#include "../../include/frr.h"

namespace frr {

struct Rule { int code; const char *msg; };   // FRR_OK: the arguments pass (no text)
constexpr Rule RULE_OK = {FRR_OK, nullptr};

// The inputs of one geometry pass -- a mesh's triangles, the (instance, triangle) pairs of an instanced pass, the sum over
// a draw list's items -- stay below this: the order key of an input's setup triangles is 32 * input + (0 .. 31), the low
// FAN_BITS = 5 bits of 32 (frr_device.h; frr_api.hip asserts the relation where it sees both).
constexpr int PASS_ORDER_KEY_BITS = 32;
constexpr int PASS_FAN_BITS = 5;
constexpr uint64_t MAX_PASS_INPUTS = 1ull << (PASS_ORDER_KEY_BITS - PASS_FAN_BITS);   // 2^27

// ---- the window rule ---------------------------------------------------------------------------------------------------
// WINDOW_RASTER   the ranges of frr_raster / frr_draw*: the reference's width_range, height_range.  x0 < 0 is fine (rows
//                 then share depth entries, as they do in the reference), and so is an empty window: a valid call that
//                 draws nothing, whatever its x1.
// WINDOW_ENTRIES  the window of the commands that address a buffer entry by entry, (cy - y0) * x1 + (cx - x0):
//                 frr_resolve_varyings, frr_readback_varyings, frr_visible_pixels*, frr_shade_varyings*.  An entry has to
//                 be one pixel's: no x0 < 0, and nothing to do is an error of the caller's, not a frame without triangles.
// Coordinates outside the i16 range (the tile kernel's packed boxes) answer FRR_ERR_UNSUPPORTED for a raster window and
// FRR_ERR_INVALID for an entry window.  The difference is deliberate and documented (include/frr.h: "a window beyond what
// frr_raster accepts" is FRR_ERR_INVALID for the entry commands); each kind also keeps the order of its checks.
enum WindowUse { WINDOW_RASTER, WINDOW_ENTRIES };

inline Rule window_rule(WindowUse use, uint32_t W, uint32_t H, int32_t x0, int32_t x1, int32_t y0, int32_t y1)
{
    const int64_t ww = (int64_t)x1 - x0, wh = (int64_t)y1 - y0;
    const Rule larger = {FRR_ERR_INVALID, "window larger than the FrameBuffer"};
    const Rule depth_index = {FRR_ERR_INVALID, "depth index (cy-y0)*x1+(cx-x0) would leave the depth buffer (renderer.rs:362)"};
    const bool in_i16 = x0 >= -32768 && y0 >= -32768 && x1 <= 32767 && y1 <= 32767;
    // the last entry the window addresses, + 1 (asked only behind the size and i16 checks: no overflow)
    const auto last_index = [&] { return (wh - 1) * (int64_t)x1 + ww; };
    const int64_t entries = (int64_t)W * (int64_t)H;
    if (use == WINDOW_RASTER) {
        if (x0 > x1 || y0 > y1) return {FRR_ERR_INVALID, "range min > max (i32::clamp would panic, renderer.rs:285)"};
        if (ww > (int64_t)W || wh > (int64_t)H) return larger;
        if (!in_i16) return {FRR_ERR_UNSUPPORTED, "window coordinates outside the i16 range"};
        if (ww > 0 && wh > 0 && (x1 <= 0 || last_index() > entries)) return depth_index;
        return RULE_OK;
    }
    if (x1 <= x0 || y1 <= y0) return {FRR_ERR_INVALID, "empty or inverted window"};
    if (x0 < 0) return {FRR_ERR_UNSUPPORTED, "x0 < 0: pixels of neighbouring rows share depth entries, an entry has no single pixel"};
    if (ww > (int64_t)W || wh > (int64_t)H) return larger;
    if (!in_i16) return {FRR_ERR_INVALID, "window coordinates outside the i16 range"};
    if (last_index() > entries) return depth_index;
    return RULE_OK;
}

// ---- the pixel-shader rule ---------------------------------------------------------------------------------------------
// K_OF_GEOMETRY  frr_raster / frr_draw*: K is what the latest geometry pass's vertex shader writes.
// K_OF_BUFFER    frr_shade_varyings*: K is what the caller says its buffer holds, so it has to be a K at all, and
//                FRR_PS_DEPTH has nothing to shade.
// K_OF_NOTHING   frr_raster / frr_draw_list* of a list without items: the pass has no vertex shader and shades nothing, so
//                there is no K and no texture a pixel shader could miss -- the id still has to name a shader.
// FRR_PS_COLOR reads three varyings, FRR_PS_PHONG / FRR_PS_BLINN eight and the texture of uniforms.texture_slot,
// FRR_PS_DEPTH / FRR_PS_FLAT none (any K goes); a user pixel shader needs the K it was registered with -- `user_K`, which
// frr_api.hip looks up (USER_K_UNKNOWN: nobody registered that id; ignored for a built-in ps_id).
enum VaryingsFrom { K_OF_GEOMETRY, K_OF_BUFFER, K_OF_NOTHING };
constexpr int USER_K_UNKNOWN = -1;

inline Rule pixel_shader_rule(VaryingsFrom from, int ps_id, int K, int user_K, bool texture_bound)
{
    const bool buffer = from == K_OF_BUFFER, nothing = from == K_OF_NOTHING;
    const bool lit = ps_id == FRR_PS_PHONG || ps_id == FRR_PS_BLINN;
    if (ps_id >= FRR_SHADER_USER_BASE) {
        if (user_K == USER_K_UNKNOWN) return {FRR_ERR_INVALID, "unknown shader id"};
        if (user_K != K && !nothing)
            return {FRR_ERR_INVALID, buffer ? "the user pixel shader's varyings do not match the buffer's K"
                                            : "the user pixel shader's varyings do not match the vertex shader's"};
    } else {
        if (buffer && ps_id == FRR_PS_DEPTH) return {FRR_ERR_INVALID, "FRR_PS_DEPTH: nothing to shade"};
        const bool bad_K = buffer && (K < 0 || K > FRR_MAX_VARYINGS);
        const bool other_K = !nothing && ((ps_id == FRR_PS_COLOR && K != 3) || (lit && K != 8));
        if (ps_id < 0 || ps_id > FRR_PS_BLINN || bad_K || other_K)
            return {FRR_ERR_INVALID, buffer    ? "pixel shader does not match the buffer's K"
                                     : nothing ? "unknown shader id"
                                               : "pixel shader does not match the vertex shader's varyings"};
    }
    if (lit && !texture_bound && !nothing) return {FRR_ERR_INVALID, "no texture bound to uniforms.texture_slot"};
    return RULE_OK;
}

// ---- the buffer rule ---------------------------------------------------------------------------------------------------
// The caller's buffer of a command with an entry window (which has passed window_rule: y1 > y0, x1 > 0): 4-byte aligned
// and, where the window's entries index it, at least (y1 - y0) * x1 entries long.
// BUFFER_VARYINGS_OUT  frr_resolve_varyings / frr_readback_varyings: [entries][K] floats, never NULL.
// BUFFER_COUNTS_OUT    frr_visible_pixels*: one u32 per unit, as many as the caller likes; with no entries nothing is
//                      written and any pointer goes.
// BUFFER_VARYINGS_IN   frr_shade_varyings*: [entries][K] floats; NULL only where K == 0 (FRR_PS_FLAT reads nothing).
enum BufferUse { BUFFER_VARYINGS_OUT, BUFFER_COUNTS_OUT, BUFFER_VARYINGS_IN };

inline Rule buffer_rule(BufferUse use, const void *buf, uint64_t entries, int K, int32_t x1, int32_t y0, int32_t y1)
{
    const bool in = use == BUFFER_VARYINGS_IN;
    const bool null_ok = in && K <= 0;
    const bool unused = use == BUFFER_COUNTS_OUT && entries == 0;
    if (!unused && ((!buf && !null_ok) || ((uintptr_t)buf & 3u)))
        return {FRR_ERR_INVALID, in ? "varyings buffer is NULL or not 4-byte aligned" : "output buffer is NULL or not 4-byte aligned"};
    if (use != BUFFER_COUNTS_OUT && entries < (uint64_t)((int64_t)y1 - y0) * (uint64_t)x1)
        return {FRR_ERR_INVALID, in ? "in_entries < (y1 - y0) * x1" : "out_entries < (y1 - y0) * x1"};
    return RULE_OK;
}

// ---- the keep rule -----------------------------------------------------------------------------------------------------
// The caller's buffer of a predicated list pass (frr_geometry_list_if / frr_draw_list_if): one u32 per item of the list, in
// device memory.  Item i is kept iff keep[i] >= min_value, compared as unsigned -- item_kept, the one comparison the device
// (k_item_keep) and the CPU test share.  Entries at and beyond the list's item count are ignored; a list without items
// reads nothing, so NULL is fine there -- a misaligned pointer never is.
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define FRR_RULE_HD __host__ __device__
#else
#define FRR_RULE_HD
#endif
FRR_RULE_HD inline bool item_kept(uint32_t value, uint32_t min_value) { return value >= min_value; }

// ---- the depth test ----------------------------------------------------------------------------------------------------
// A fragment passes iff `rhw < depth` is false (renderer.rs:363): a tie passes, and so does everything where either side is
// NaN.  The one comparison frr_query_pixels' kernel (frr_query.h) and the CPU test share.
FRR_RULE_HD inline bool fragment_passes(float rhw, float depth) { return !(rhw < depth); }

inline Rule keep_rule(const void *keep, uint64_t keep_entries, uint64_t nitems)
{
    if ((!keep && nitems > 0) || ((uintptr_t)keep & 3u)) return {FRR_ERR_INVALID, "keep buffer is NULL or not 4-byte aligned"};
    if (keep_entries < nitems) return {FRR_ERR_INVALID, "keep_entries < the list's item count"};
    return RULE_OK;
}

// ---- the box rules -----------------------------------------------------------------------------------------------------
// bounds_rule  frr_drawlist_bounds: the object-space box of an item's mesh bounds what the item draws only where the vertex
//              shader is position -> mvp * position: FRR_VS_PHONG and FRR_VS_GOURAUD.  The inputs of FRR_VS_CLIP* are clip
//              coordinates (there is no object space), and a user vertex shader may move a vertex anywhere.
// boxes_rule   frr_query_boxes*: the list has a bounds table (frr_drawlist_bounds succeeded on it since its upload).  Its
//              window is a WINDOW_ENTRIES window, its buffer a BUFFER_COUNTS_OUT buffer.
inline Rule bounds_rule(int vs_id)
{
    if (vs_id == FRR_VS_PHONG || vs_id == FRR_VS_GOURAUD) return RULE_OK;
    if (vs_id >= FRR_SHADER_USER_BASE) return {FRR_ERR_UNSUPPORTED, "frr_drawlist_bounds: a user vertex shader may move a vertex anywhere, a box of its inputs bounds nothing"};
    return {FRR_ERR_UNSUPPORTED, "frr_drawlist_bounds: the inputs of FRR_VS_CLIP* are clip coordinates, there is no object space"};
}
inline Rule boxes_rule(bool has_bounds)
{
    if (!has_bounds) return {FRR_ERR_INVALID, "the draw list has no bounds table: call frr_drawlist_bounds first"};
    return RULE_OK;
}

// ---- the materials rule ------------------------------------------------------------------------------------------------
// A table of frr_material (frr_materials_upload / frr_materials_bind_device) and its use by frr_shade_items*.
// material_ok    one entry: texture_slot in 0 .. FRR_MAX_TEXTURES-1 and reserved == 0 -- the one test the host (upload) and
//                the device (k_materials_check, at bind) share.  NaN and infinite values are not refused.
// MATERIALS_UPLOAD / MATERIALS_BIND   the table's pointer: NULL only for n == 0; a device-bound table is read with
//                16-byte loads, so a pointer that is not 16-byte aligned never passes -- a host array may lie anywhere.
// MATERIALS_SHADE  the table against the pass at the call: at least one entry per item of the latest geometry pass (more
//                are fine, the rest is ignored; `n` entries, `nitems` items), and -- lit: FRR_PS_PHONG / FRR_PS_BLINN, which
//                sample the material's slot -- every slot the table names (`slots`, bit s: some entry has texture_slot s)
//                holds a texture (`filled`, bit s: slot s does).  A user pixel shader samples an empty slot as zero
//                (the kernel gives such a material a 1 x 1 texture of zeros: frr_shade.h, material_apply).
// *which: the first slot a lit shader would miss (frr_api.hip names it in frr_last_error); untouched otherwise.
FRR_RULE_HD inline bool material_ok(const frr_material &m) { return m.texture_slot >= 0 && m.texture_slot < FRR_MAX_TEXTURES && m.reserved == 0; }

enum MaterialsUse { MATERIALS_UPLOAD, MATERIALS_BIND, MATERIALS_SHADE };

inline Rule materials_rule(MaterialsUse use, const void *mats, uint64_t n, uint64_t nitems = 0, bool lit = false, uint32_t slots = 0, uint32_t filled = 0,
                           int *which = nullptr)
{
    if (use == MATERIALS_SHADE) {
        if (n < nitems) return {FRR_ERR_INVALID, "the material table has fewer entries than the latest geometry pass has items"};
        const uint32_t missing = lit ? slots & ~filled : 0u;
        if (missing) {
            if (which) { int s = 0; while (!((missing >> s) & 1u)) ++s; *which = s; }
            return {FRR_ERR_INVALID, "a material names a texture slot that holds no texture"};
        }
        return RULE_OK;
    }
    if (!mats && n > 0) return {FRR_ERR_INVALID, "material table is NULL"};
    if (use == MATERIALS_BIND && ((uintptr_t)mats & 15u)) return {FRR_ERR_INVALID, "material table pointer must be 16-byte aligned"};
    return RULE_OK;
}

} // namespace frr
