"""CPU: the host's rule for which raster passes are known to fit the work lists and are not waited for (DESIGN.md section 1a,
f_renderer_amd/csrc/frr_proof.h), compiled with the host compiler and run: a signature is known once it was added and not
before; any single field of it that differs -- of what the geometry pass read or of the raster pass's own facts -- makes it
unknown; the set keeps the latest 32; a predicated pass is never known and never entered; and two signatures built from the
same facts compare equal whatever the memory they were built in held before.  The same program under the host compiler's
address and undefined-behaviour sanitizers ends clean with the same answers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "frr_proof.h"
#include <stdio.h>
#include <new>
using namespace frr;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

static const float kMesh[2] = {0.0f, 0.0f}, kInst[2] = {0.0f, 0.0f};
static GeomRead some_read()
{
    GeomRead r;
    r.mesh = kMesh; r.mesh_gen = 3; r.ntris = 1000; r.duni_hash = 0x1234567890abcdefull;
    r.inst = kInst; r.inst_gen = 2; r.ninst = 7; r.tex_epoch = 4; r.sync_epoch = 5; r.list_gen = 6;
    r.vs = 2; r.cull = 1; r.list = 9; r.filter = 1; r.fy0 = 0; r.fy1 = 1080;
    return r;
}
static DrawSig some_sig(const GeomRead &r) { return draw_sig(r, 0, 1920, 0, 1080, 3, 8, true, 1, 0, 11u); }

// One walk over every field of both structs: `change` gives the field another value, and the sizes of the fields walked are
// summed -- the structs have no padding (frr_proof.h asserts it), so a field without a line here leaves the sum short of sizeof.
static size_t walked;
template <typename T> static void bump(T &v) { v += 1; walked += sizeof v; }
static void bump(const float *&p) { p += 1; walked += sizeof p; }
static int change(DrawSig &s, int f)
{
    GeomRead &r = s.read;
    switch (f) {
    case 0: bump(r.mesh); break;       case 1: bump(r.mesh_gen); break;   case 2: bump(r.ntris); break;
    case 3: bump(r.duni_hash); break;  case 4: bump(r.inst); break;       case 5: bump(r.inst_gen); break;
    case 6: bump(r.ninst); break;      case 7: bump(r.tex_epoch); break;  case 8: bump(r.sync_epoch); break;
    case 9: bump(r.list_gen); break;   case 10: bump(r.vs); break;        case 11: bump(r.cull); break;
    case 12: bump(r.list); break;      case 13: bump(r.filter); break;    case 14: bump(r.fy0); break;
    case 15: bump(r.fy1); break;
    case 16: bump(s.x0); break;        case 17: bump(s.x1); break;        case 18: bump(s.y0); break;
    case 19: bump(s.y1); break;        case 20: bump(s.rank); break;      case 21: bump(s.world); break;
    case 22: bump(s.blocked); break;   case 23: bump(s.gset); break;      case 24: bump(s.bset); break;
    case 25: bump(s.join_epoch); break;
    default: return 0;
    }
    return 1;
}
constexpr int kReadFields = 16;

int main()
{
    const DrawSig k = some_sig(some_read());
    ProvenSet set;
    CHECK(!set.known(k, false));                       // unknown before it is added ...
    set.add(k, false);
    CHECK(set.known(k, false) && set.size() == 1);     // ... and known after

    // any single field that differs: unknown
    int nfields = 0;
    size_t read_bytes = 0;
    for (int f = 0;; ++f) {
        DrawSig p = k;
        if (!change(p, f)) break;
        ++nfields;
        if (nfields == kReadFields) read_bytes = walked;
        CHECK(!same_sig(p, k));
        CHECK(!set.known(p, false));
        set.add(p, false);
        CHECK(set.known(p, false) && set.known(k, false));
    }
    CHECK(nfields == 26);
    CHECK(read_bytes == sizeof(GeomRead));             // every field of both structs was walked
    CHECK(walked == sizeof(DrawSig));
    CHECK(draw_sig(k.read, 0, 1920, 0, 1080, 3, 8, false, 1, 0, 11u).blocked == 0 && k.blocked == 1);

    // 33 distinct signatures: the first is forgotten, the other 32 are known
    set.clear();
    CHECK(set.size() == 0 && !set.known(k, false));    // clear() empties it
    DrawSig d = k;
    for (int i = 0; i < ProvenSet::CAPACITY + 1; ++i) { d.read.mesh_gen = 100 + i; set.add(d, false); }
    CHECK(ProvenSet::CAPACITY == 32 && set.size() == 32);
    d.read.mesh_gen = 100;
    CHECK(!set.known(d, false));
    for (int i = 1; i < ProvenSet::CAPACITY + 1; ++i) { d.read.mesh_gen = 100 + i; CHECK(set.known(d, false)); }
    // ... and oldest first from then on: two more push out 101 and 102, and nothing else
    for (int i = 33; i < 35; ++i) { d.read.mesh_gen = 100 + i; set.add(d, false); }
    for (int i = 0; i < 35; ++i) { d.read.mesh_gen = 100 + i; CHECK(set.known(d, false) == (i >= 3)); }

    // a predicated pass is never known, even when the same signature was added unpredicated, and adds nothing
    set.clear();
    set.add(k, true);
    CHECK(set.size() == 0 && !set.known(k, false) && !set.known(k, true));
    set.add(k, false);
    CHECK(set.known(k, false) && !set.known(k, true));
    set.add(d, true);
    CHECK(set.size() == 1 && !set.known(d, false) && set.known(k, false));
    set.clear();
    CHECK(set.size() == 0 && !set.known(k, false));

    // the padding case: the same facts through separately constructed, struct-copied GeomRead values, in memory that held
    // different bytes before, give equal signatures
    struct Holder { char pad; GeomRead r; };           // (what a GeomRead kept inside a larger, copied struct goes through)
    alignas(Holder) unsigned char ma[sizeof(Holder)], mb[sizeof(Holder)];
    alignas(DrawSig) unsigned char sa[sizeof(DrawSig)], sb[sizeof(DrawSig)];
    memset(ma, 0x00, sizeof ma); memset(mb, 0xFF, sizeof mb); memset(sa, 0x55, sizeof sa); memset(sb, 0xAA, sizeof sb);
    Holder *ha = new (ma) Holder, *hb = new (mb) Holder;
    ha->r = some_read();
    { GeomRead t = some_read(); Holder h2; h2.pad = 1; h2.r = t; *hb = h2; }
    DrawSig *pa = new (sa) DrawSig(some_sig(ha->r)), *pb = new (sb) DrawSig(some_sig(hb->r));
    CHECK(same_sig(*pa, *pb) && same_sig(*pa, k));
    set.add(*pa, false);
    CHECK(set.known(*pb, false));

    printf("%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}
"""


def build(tmp_path, name, flags=()):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = tmp_path / "proof.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "f_renderer_amd", "csrc"),
                        "-o", str(exe), str(src)], capture_output=True, text=True)
    return exe if p.returncode == 0 else None, p.stderr


def test_proof_rule(tmp_path):
    exe, err = build(tmp_path, "proof")
    assert exe is not None, err
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "OK", p.stdout + p.stderr


def test_proof_rule_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same program -- host code with its own main -- built with -fsanitize=address,undefined -fno-sanitize-recover=all: it
    ends clean, with the answers of the plain build.  (Skipped where the host compiler has no sanitizer runtime to link.)"""
    plain, err = build(tmp_path, "proof")
    assert plain is not None, err
    exe, _ = build(tmp_path, "proof_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if exe is None:
        pytest.skip("the host compiler's sanitizer runtimes are not installed")
    a = subprocess.run([str(plain)], capture_output=True, text=True)
    b = subprocess.run([str(exe)], capture_output=True, text=True)
    assert b.returncode == 0 and b.stdout == a.stdout and b.stdout.strip() == "OK", b.stdout + b.stderr
