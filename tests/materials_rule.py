"""The materials rule of f_renderer_amd/csrc/frr_rules.h -- material_ok, the test of one entry the host (upload) and the
device (k_materials_check, at bind) share, and materials_rule, the argument rule of frr_materials_upload /
frr_materials_bind_device / frr_shade_items -- as a host program with its own main: built once per session with the host
compiler, the way tests/keep_rule.py builds the keep rule, and asked over stdin, one query per line, one answer line each:
  m texture_slot reserved                               material_ok      -> "1\t" or "0\t"
  t use pointer n nitems lit slots filled               materials_rule   -> "<status code>\t<text>|<which>"
(use: 0 upload, 1 bind, 2 shade; text empty where the rule passes; which: the slot a lit shader misses, else -1)"""
import functools
import os
import subprocess

from . import arg_rules as R

OK, INVALID = R.OK, R.INVALID
UPLOAD, BIND, SHADE = 0, 1, 2

PROGRAM = r"""
#include "frr_rules.h"
#include <stdio.h>
#include <inttypes.h>
#include <string.h>
using namespace frr;
int main()
{
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'm') {
            frr_material m;
            memset(&m, 0xA5, sizeof m);   // (every other field is rubbish: the test reads two)
            if (scanf("%" SCNd32 " %" SCNd32, &m.texture_slot, &m.reserved) != 2) return 2;
            printf("%d\t\n", material_ok(m) ? 1 : 0);
        } else if (kind == 't') {
            int use, lit; uint64_t ptr, n, nitems; uint32_t slots, filled;
            if (scanf("%d %" SCNu64 " %" SCNu64 " %" SCNu64 " %d %" SCNu32 " %" SCNu32, &use, &ptr, &n, &nitems, &lit, &slots, &filled) != 7) return 2;
            int which = -1;
            const Rule r = materials_rule(use == 0 ? MATERIALS_UPLOAD : use == 1 ? MATERIALS_BIND : MATERIALS_SHADE, (const void *)(uintptr_t)ptr, n, nitems,
                                          lit != 0, slots, filled, &which);
            printf("%d\t%s|%d\n", r.code, r.msg ? r.msg : "", which);
        } else return 2;
    }
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def build(flags=()):
    """The program, built with extra `flags`; None where the flagged build fails because the sanitizer's runtime is not
    installed (the linker cannot find it) -- any other build error fails the caller."""
    cxx = R.compiler()
    assert cxx is not None, "no host C++ compiler"
    d = R._workdir()
    src = os.path.join(d, "materials.cpp")
    with open(src, "w") as fh:
        fh.write(PROGRAM)
    exe = os.path.join(d, "materials" + str(len(os.listdir(d))))
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(R.ROOT, "f_renderer_amd", "csrc"), "-o", exe, src],
                       capture_output=True, text=True)
    if p.returncode != 0:
        missing_runtime = "cannot find" in p.stderr and "san" in p.stderr     # ld: cannot find -lubsan / libubsan.so ...
        assert flags and missing_runtime, p.stderr
        return None
    return exe


def ask(lines, exe=None):
    return R.ask(lines, exe or build())


def ok(slot, reserved):
    return f"m {slot} {reserved}"


def table(use, ptr, n, nitems=0, lit=False, slots=0, filled=0):
    return f"t {use} {ptr} {n} {nitems} {int(lit)} {slots} {filled}"
