"""The keep rule of f_renderer_amd/csrc/frr_rules.h -- item_kept, the comparison the device's k_item_keep evaluates, and
keep_rule, the argument rule of frr_geometry_list_if / frr_draw_list_if -- as a host program with its own main: built once per
session with the host compiler, the way tests/arg_rules.py builds the other rules, and asked over stdin, one query per line,
one answer line each:
  k value min_value                 item_kept   -> "1\t" or "0\t"
  r pointer keep_entries nitems     keep_rule   -> "<status code>\t<text>" (text empty where the rule passes)"""
import functools
import os
import subprocess

from . import arg_rules as R

OK, INVALID = R.OK, R.INVALID

PROGRAM = r"""
#include "frr_rules.h"
#include <stdio.h>
#include <inttypes.h>
using namespace frr;
int main()
{
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'k') {
            uint32_t value, min_value;
            if (scanf("%" SCNu32 " %" SCNu32, &value, &min_value) != 2) return 2;
            printf("%d\t\n", item_kept(value, min_value) ? 1 : 0);
        } else if (kind == 'r') {
            uint64_t ptr, entries, nitems;
            if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &ptr, &entries, &nitems) != 3) return 2;
            const Rule r = keep_rule((const void *)(uintptr_t)ptr, entries, nitems);
            printf("%d\t%s\n", r.code, r.msg ? r.msg : "");
        } else return 2;
    }
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def build(flags=()):
    """The program, built with extra `flags`; None where the build fails (asked for by the sanitizer build alone)."""
    cxx = R.compiler()
    assert cxx is not None, "no host C++ compiler"
    d = R._workdir()
    src = os.path.join(d, "keep.cpp")
    with open(src, "w") as fh:
        fh.write(PROGRAM)
    exe = os.path.join(d, "keep" + str(len(os.listdir(d))))
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(R.ROOT, "f_renderer_amd", "csrc"), "-o", exe, src],
                       capture_output=True, text=True)
    if p.returncode != 0:
        assert flags, p.stderr
        return None
    return exe


def ask(lines, exe=None):
    return R.ask(lines, exe or build())


def kept(value, min_value):
    return f"k {value} {min_value}"


def rule(ptr, entries, nitems):
    return f"r {ptr} {entries} {nitems}"
