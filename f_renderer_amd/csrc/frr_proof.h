// frr_proof.h -- host side of "a draw cannot fail" (DESIGN.md section 1a): which raster passes are known to fit the work
// lists, so that the host need not wait for them?  Plain C++ (no HIP), so that a CPU test can hold the rule
// (tests/test_proof_rule_cpu.py).
//
// A raster pass whose need of the work lists (fan space, (triangle, tile) records) is not known to fit is verified before
// frr_raster returns.  It is known to fit if a pass with the same signature (DrawSig) has completed on the current lists:
// the set of those signatures is the ProvenSet.
#pragma once
#include <stdint.h>
#include <string.h>

#include <type_traits>

namespace frr {

// What decides how much of the work lists (fan space, (triangle, tile) records) a raster pass and its geometry pass need.
// Everything the geometry pass reads can change what it emits: the mesh (its registration, and for a device-bound one the
// frr_sync calls since -- the caller may rewrite it in place then), the uniforms (a user VS may read any field, texture
// pointers and sizes included) and the texture contents (frr_texture_upload count).
// So can the cull mode (frr_set_cull): a pass proven to fit under one mode says nothing about another.
// (An indexed mesh needs no field of its own: its index list and vertex count belong to its registration, mesh_gen, and
// binding it again after a rewrite is a new registration.)
//
// GeomRead: what a geometry pass read -- everything that decides what it emits.  The pass fills it once (exec_geometry), and
// the signature of every raster pass over its setup list takes it whole.
struct GeomRead {
    const float *mesh = nullptr; uint64_t mesh_gen = 0, ntris = 0;   // the mesh, which registration of the ctx it is, and the pass's inputs
    uint64_t duni_hash = 0;                                          // a digest of its uniforms
    const float *inst = nullptr; uint64_t inst_gen = 0, ninst = 0;   // an instanced pass: its table (bound again, or device-bound and behind a frr_sync: unproven again, like a mesh)
    uint64_t tex_epoch = 0, sync_epoch = 0;                          // the texture uploads and (device-bound inputs) the frr_sync calls before it
    uint64_t list_gen = 0;   // a list pass: which upload its id meant -- a pass proven for one list says nothing about a later list with that id
    int32_t vs = -1;         // its vertex shader (< 0: no pass yet)
    int32_t cull = 0;        // the cull mode it ran under (FRR_CULL_NONE)
    int32_t list = -1;       // a list pass: its list
    int32_t filter = 0, fy0 = 0, fy1 = 0;   // frr_draw on a partitioned ctx: the setup list holds only the triangles of the rank's tile rows of window rows fy0 .. fy1
};

// ... and the raster pass's own facts: window, tile-row ownership, the workspace sets of the two passes, the bind epoch.
struct DrawSig {
    GeomRead read;
    int32_t x0, x1, y0, y1;
    int32_t rank, world, blocked;
    int32_t gset, bset;
    uint32_t join_epoch;
};
// same_sig compares the bytes, and GeomRead travels by struct copy: neither struct may hold a byte no field owns
static_assert(std::has_unique_object_representations_v<GeomRead> && std::has_unique_object_representations_v<DrawSig>, "a signature has no padding");

inline DrawSig draw_sig(const GeomRead &read, int32_t x0, int32_t x1, int32_t y0, int32_t y1, int rank, int world, bool blocked, int gset, int bset, uint32_t join_epoch)
{
    return DrawSig{read, x0, x1, y0, y1, rank, world, blocked ? 1 : 0, gset, bset, join_epoch};
}
inline bool same_sig(const DrawSig &a, const DrawSig &b) { return memcmp(&a, &b, sizeof a) == 0; }

// The signatures of the passes that have completed on the current lists: the latest 32, oldest out first.
// A predicated pass is never known and never entered: which items it keeps is device data, so neither its own earlier runs
// nor the unpredicated pass over the same list say what it needs -- and it proves nothing for anybody else.
// (A replay never asks: its passes are waited for by finish().)
class ProvenSet {
public:
    static constexpr int CAPACITY = 32;
    bool known(const DrawSig &sig, bool predicated) const
    {
        if (predicated) return false;
        for (int i = 0; i < n_; ++i) if (same_sig(sigs_[i], sig)) return true;
        return false;
    }
    void add(const DrawSig &sig, bool predicated)
    {
        if (predicated) return;
        if (n_ < CAPACITY) { sigs_[n_++] = sig; return; }
        sigs_[oldest_] = sig;
        oldest_ = (oldest_ + 1) % CAPACITY;
    }
    void clear() { n_ = oldest_ = 0; }
    int size() const { return n_; }
private:
    DrawSig sigs_[CAPACITY];
    int n_ = 0, oldest_ = 0;   // sigs_[oldest_] is the next to go once the set is full
};

} // namespace frr
