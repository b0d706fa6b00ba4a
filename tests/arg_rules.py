"""The argument rules of f_renderer_amd/csrc/frr_rules.h as a host program: built once per session with the host compiler
(as tests/test_tile_order_rule.py builds its rule) and asked over stdin, one query per line, one answer line each:
  w <use> W H x0 x1 y0 y1                       window_rule        (use: 0 raster, 1 entries)
  p <from> ps_id K user_K texture               pixel_shader_rule  (from: 0 geometry, 1 buffer, 2 nothing; user_K -1: unknown id)
  b <use> pointer entries K x1 y0 y1            buffer_rule        (use: 0 varyings out, 1 counts out, 2 varyings in)
  c                                             MAX_PASS_INPUTS
The answer is "<status code>\t<text>" (text empty where the rule passes)."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -4
RASTER, ENTRIES = 0, 1
FROM_GEOMETRY, FROM_BUFFER, FROM_NOTHING = 0, 1, 2
VARYINGS_OUT, COUNTS_OUT, VARYINGS_IN = 0, 1, 2
USER_K_UNKNOWN = -1

PROGRAM = r"""
#include "frr_rules.h"
#include <stdio.h>
#include <inttypes.h>
using namespace frr;
static void answer(const Rule &r) { printf("%d\t%s\n", r.code, r.msg ? r.msg : ""); }
int main()
{
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'w') {
            int use; uint32_t W, H; int32_t x0, x1, y0, y1;
            if (scanf("%d %" SCNu32 " %" SCNu32 " %" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd32, &use, &W, &H, &x0, &x1, &y0, &y1) != 7) return 2;
            answer(window_rule(use ? WINDOW_ENTRIES : WINDOW_RASTER, W, H, x0, x1, y0, y1));
        } else if (kind == 'p') {
            int from, ps, K, user_K, tex;
            if (scanf("%d %d %d %d %d", &from, &ps, &K, &user_K, &tex) != 5) return 2;
            answer(pixel_shader_rule(from == 0 ? K_OF_GEOMETRY : from == 1 ? K_OF_BUFFER : K_OF_NOTHING, ps, K, user_K, tex != 0));
        } else if (kind == 'b') {
            int use, K; uint64_t ptr, entries; int32_t x1, y0, y1;
            if (scanf("%d %" SCNu64 " %" SCNu64 " %d %" SCNd32 " %" SCNd32 " %" SCNd32, &use, &ptr, &entries, &K, &x1, &y0, &y1) != 7) return 2;
            answer(buffer_rule(use == 0 ? BUFFER_VARYINGS_OUT : use == 1 ? BUFFER_COUNTS_OUT : BUFFER_VARYINGS_IN, (const void *)(uintptr_t)ptr, entries, K, x1, y0, y1));
        } else if (kind == 'c') {
            printf("%" PRIu64 "\t\n", (uint64_t)MAX_PASS_INPUTS);
        } else return 2;
    }
    return 0;
}
"""

_dir = None


def _workdir():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="frr_rules_")
        atexit.register(shutil.rmtree, _dir, ignore_errors=True)
    return _dir


def compiler():
    return shutil.which("g++") or shutil.which("c++")


@functools.lru_cache(maxsize=None)
def build(flags=()):
    """The program, built with extra `flags`; None where the build fails (asked for by the sanitizer build alone)."""
    cxx = compiler()
    assert cxx is not None, "no host C++ compiler"
    d = _workdir()
    src = os.path.join(d, "rules.cpp")
    with open(src, "w") as fh:
        fh.write(PROGRAM)
    exe = os.path.join(d, "rules" + str(len(os.listdir(d))))
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "f_renderer_amd", "csrc"), "-o", exe, src],
                       capture_output=True, text=True)
    if p.returncode != 0:
        assert flags, p.stderr
        return None
    return exe


def ask(lines, exe=None):
    """[(code, text)] of the queries `lines`"""
    lines = list(lines)
    p = subprocess.run([exe or build()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(lines), (len(out), len(lines))
    return [(int(a), b) for a, b in (o.split("\t", 1) for o in out)]


def window(use, W, H, x0, x1, y0, y1):
    return f"w {use} {W} {H} {x0} {x1} {y0} {y1}"


def shader(frm, ps, K, user_K, tex):
    return f"p {frm} {ps} {K} {user_K} {int(tex)}"


def buffer(use, ptr, entries, K, x1, y0, y1):
    return f"b {use} {ptr} {entries} {K} {x1} {y0} {y1}"
