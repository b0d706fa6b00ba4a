"""CPU: the argument rules of the commands (f_renderer_amd/csrc/frr_rules.h), compiled with the host compiler and asked
through tests/arg_rules.py.  The raster window rule against the C oracle on every window around three small FrameBuffers;
the entry window rule against what it promises (one pixel per entry, inside the buffer); codes and precedence at the i16
and i32 edges; the pixel-shader rule's whole truth table against the rule as include/frr.h words it; the buffer rule.
The same queries go through a build with the host compiler's undefined-behaviour sanitizer where its runtime exists."""
import itertools

import numpy as np
import pytest

from . import arg_rules as R
from .arg_rules import ENTRIES, FROM_BUFFER, FROM_GEOMETRY, INVALID, OK, RASTER, UNSUPPORTED

SIZES = [(5, 4), (8, 3), (3, 6)]
INVERTED = {(5, 4): 12276, (8, 3): 15900, (3, 6): 11895}     # windows of the grid with x0 > x1 or y0 > y1
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
PS_DEPTH, PS_FLAT, PS_COLOR, PS_PHONG, PS_BLINN = range(5)
USER, MAX_VARYINGS = 64, 16
EW, EH = 64, 48

# two triangles that cover the whole viewport (VS_CLIP)
QUAD = np.array([[[-1, -1, .5, 1], [1, -1, .5, 1], [1, 1, .5, 1]], [[-1, -1, .5, 1], [1, 1, .5, 1], [-1, 1, .5, 1]]], np.float32)


def grid(W, H):
    xs, ys = range(-3, W + 4), range(-3, H + 4)
    return [(x0, x1, y0, y1) for x0 in xs for x1 in xs for y0 in ys for y1 in ys]


def grid_queries():
    return [R.window(use, W, H, *w) for W, H in SIZES for use in (RASTER, ENTRIES) for w in grid(W, H)]


@pytest.mark.parametrize("W,H", SIZES)
def test_raster_window_rule_against_the_oracle(oracle, W, H):
    """Wherever the raster rule accepts a window, drawing or not, the oracle completes a draw that covers the viewport;
    and the rule answers "min > max" exactly on the windows with x0 > x1 or y0 > y1, every one of which the oracle
    refuses (i32::clamp, renderer.rs:285).  Not the converse: the rule is stricter than the reference elsewhere."""
    wins = grid(W, H)
    got = R.ask(R.window(RASTER, W, H, *w) for w in wins)
    f = oracle.Frame(W, H)
    uni = oracle.make_uniforms()
    panics_accepted, inverted, inverted_refused = [], 0, 0
    for w, (code, text) in zip(wins, got):
        try:
            f.draw(QUAD, oracle.VS_CLIP, oracle.PS_FLAT, uni, window=w)
            completed = True
        except RuntimeError:
            completed = False
        if code == OK and not completed:
            panics_accepted.append(w)
        inv = w[0] > w[1] or w[2] > w[3]
        assert ("min > max" in text) == inv and (not inv or code == INVALID), (w, code, text)
        inverted += inv
        inverted_refused += inv and not completed
    assert not panics_accepted, panics_accepted[:10]
    assert inverted == inverted_refused == INVERTED[(W, H)]
    assert sum(code == OK for code, _ in got) > 100


@pytest.mark.parametrize("W,H", SIZES)
def test_entry_window_rule_gives_every_pixel_its_own_entry(W, H):
    """A window the entry rule accepts is accepted by the raster rule, is non-empty with x0 >= 0, and maps its pixels to
    pairwise distinct depth indices (cy - y0) * x1 + (cx - x0), all below W * H."""
    wins = grid(W, H)
    entry = R.ask(R.window(ENTRIES, W, H, *w) for w in wins)
    raster = R.ask(R.window(RASTER, W, H, *w) for w in wins)
    accepted = 0
    for (x0, x1, y0, y1), (ce, _), (cr, _) in zip(wins, entry, raster):
        if ce != OK:
            continue
        accepted += 1
        assert cr == OK and x1 > x0 and y1 > y0 and x0 >= 0
        cy, cx = np.mgrid[y0:y1, x0:x1]
        idx = ((cy - y0) * x1 + (cx - x0)).ravel()
        assert idx.min() >= 0 and idx.max() < W * H and np.unique(idx).size == idx.size, (x0, x1, y0, y1)
    assert accepted > 50
    assert (OK, "") == entry[wins.index((0, W, 0, H))]


# (window on a 64 x 48 FrameBuffer, raster (code, word of its text), entries (code, word)); None: accepted
EDGES = [
    # the i16 edge in each coordinate
    ((32759, 32767, 0, EH), (INVALID, "depth index"), (INVALID, "depth index")),
    ((32760, 32768, 0, EH), (UNSUPPORTED, "i16"), (INVALID, "i16")),
    ((-32768, -32760, 0, EH), (INVALID, "depth index"), (UNSUPPORTED, "x0 < 0")),          # (raster: x1 <= 0)
    ((-32769, -32761, 0, EH), (UNSUPPORTED, "i16"), (UNSUPPORTED, "x0 < 0")),
    ((-32768, -32768 + EW, 0, EH), (INVALID, "depth index"), (UNSUPPORTED, "x0 < 0")),
    ((0, EW, -32768, -32760), None, None),
    ((0, EW, -32769, -32761), (UNSUPPORTED, "i16"), (INVALID, "i16")),
    ((0, EW, 32759, 32767), None, None),
    ((0, EW, 32760, 32768), (UNSUPPORTED, "i16"), (INVALID, "i16")),
    ((0, EW, 32767, 32768), (UNSUPPORTED, "i16"), (INVALID, "i16")),
    ((0, 32767, 0, 1), (INVALID, "larger"), (INVALID, "larger")),
    ((32767, 32767, 0, EH), None, (INVALID, "empty")),
    ((32768, 32768, 0, EH), (UNSUPPORTED, "i16"), (INVALID, "empty")),
    ((0, EW, -32768, -32768), None, (INVALID, "empty")),
    # the i32 edge: no arithmetic of the rule overflows
    ((I32_MIN, I32_MIN + 8, 0, EH), (UNSUPPORTED, "i16"), (UNSUPPORTED, "x0 < 0")),
    ((I32_MAX - 8, I32_MAX, 0, EH), (UNSUPPORTED, "i16"), (INVALID, "i16")),
    ((0, EW, I32_MIN, I32_MIN + 8), (UNSUPPORTED, "i16"), (INVALID, "i16")),
    ((0, EW, I32_MAX - 8, I32_MAX), (UNSUPPORTED, "i16"), (INVALID, "i16")),
    ((I32_MIN, EW, 0, EH), (INVALID, "larger"), (UNSUPPORTED, "x0 < 0")),
    ((I32_MAX, EW, 0, EH), (INVALID, "min > max"), (INVALID, "empty")),
    ((0, I32_MIN, 0, EH), (INVALID, "min > max"), (INVALID, "empty")),
    ((0, I32_MAX, 0, EH), (INVALID, "larger"), (INVALID, "larger")),
    ((0, EW, I32_MIN, EH), (INVALID, "larger"), (INVALID, "larger")),
    ((0, EW, I32_MAX, EH), (INVALID, "min > max"), (INVALID, "empty")),
    ((0, EW, 0, I32_MIN), (INVALID, "min > max"), (INVALID, "empty")),
    ((0, EW, 0, I32_MAX), (INVALID, "larger"), (INVALID, "larger")),
    ((I32_MIN, I32_MAX, I32_MIN, I32_MAX), (INVALID, "larger"), (UNSUPPORTED, "x0 < 0")),
    ((I32_MAX, I32_MIN, I32_MAX, I32_MIN), (INVALID, "min > max"), (INVALID, "empty")),
    ((I32_MIN, I32_MIN, I32_MIN, I32_MIN), (UNSUPPORTED, "i16"), (INVALID, "empty")),
    ((I32_MAX, I32_MAX, I32_MAX, I32_MAX), (UNSUPPORTED, "i16"), (INVALID, "empty")),
    # two rules with different codes: the one applied first answers
    ((-32769, -32769 + EW + 1, 0, EH), (INVALID, "larger"), (UNSUPPORTED, "x0 < 0")),      # raster: larger before i16; entries: x0 < 0 before larger
    ((32710, 32768, 0, EH), (UNSUPPORTED, "i16"), (INVALID, "i16")),                       # raster: i16 before the depth index
    ((32768, 32760, 0, EH), (INVALID, "min > max"), (INVALID, "empty")),                   # raster: min > max before i16
    ((-5, -5, 0, EH), None, (INVALID, "empty")),                                           # entries: empty before x0 < 0
    ((-1, EW, 0, EH), (INVALID, "larger"), (UNSUPPORTED, "x0 < 0")),
    ((-4, 60, 0, EH), None, (UNSUPPORTED, "x0 < 0")),
    ((EW, 2 * EW, 0, EH), (INVALID, "depth index"), (INVALID, "depth index")),
    ((-5, 0, 0, EH), (INVALID, "depth index"), (UNSUPPORTED, "x0 < 0")),
]


def edge_queries():
    return [R.window(use, EW, EH, *w) for w, _, _ in EDGES for use in (RASTER, ENTRIES)]


def test_window_codes_and_precedence_at_the_edges():
    got = R.ask(edge_queries())
    for k, (w, raster, entries) in enumerate(EDGES):
        for (code, text), want, kind in ((got[2 * k], raster, "raster"), (got[2 * k + 1], entries, "entries")):
            if want is None:
                assert (code, text) == (OK, ""), (kind, w, code, text)
            else:
                assert code == want[0] and want[1] in text, (kind, w, code, text, want)


def ps_cases():
    """(from, ps_id, K, user_K, texture) over the whole table"""
    shaders = [(ps, R.USER_K_UNKNOWN) for ps in range(-1, PS_BLINN + 2)] + [(USER, 3), (USER + 7, 8), (USER, R.USER_K_UNKNOWN)]
    return [(frm, ps, K, uk, tex) for frm in (FROM_GEOMETRY, FROM_BUFFER) for ps, uk in shaders
            for K in (-1, 0, 3, 8, MAX_VARYINGS + 1) for tex in (False, True)]


def ps_want(frm, ps, K, user_K, tex):
    """include/frr.h in words: FRR_PS_COLOR needs K = 3, FRR_PS_PHONG / FRR_PS_BLINN K = 8 and a texture, a user id the K it
    was registered with, the others any K; a buffer's K is 0 .. FRR_MAX_VARYINGS and FRR_PS_DEPTH has nothing to shade."""
    if ps >= USER:
        return user_K != R.USER_K_UNKNOWN and user_K == K
    if ps < 0 or ps > PS_BLINN:
        return False
    if frm == FROM_BUFFER and (ps == PS_DEPTH or not 0 <= K <= MAX_VARYINGS):
        return False
    if ps == PS_COLOR:
        return K == 3
    if ps in (PS_PHONG, PS_BLINN):
        return K == 8 and tex
    return True


def test_pixel_shader_rule_truth_table():
    cases = ps_cases()
    assert len(cases) == 2 * 10 * 5 * 2
    got = R.ask(R.shader(*c) for c in cases)
    for c, (code, text) in zip(cases, got):
        assert code == (OK if ps_want(*c) else INVALID) and (code == OK) == (text == ""), (c, code, text)
    by = dict(zip(cases, got))
    # which rule answers where two are broken: the id before the K, the K before the texture
    assert "unknown shader id" in by[(FROM_GEOMETRY, USER, 3, R.USER_K_UNKNOWN, False)][1]
    assert "texture" in by[(FROM_GEOMETRY, PS_PHONG, 8, R.USER_K_UNKNOWN, False)][1]
    assert "texture" not in by[(FROM_GEOMETRY, PS_PHONG, 3, R.USER_K_UNKNOWN, False)][1]
    assert "nothing to shade" in by[(FROM_BUFFER, PS_DEPTH, 3, R.USER_K_UNKNOWN, True)][1]
    assert by[(FROM_GEOMETRY, PS_DEPTH, 3, R.USER_K_UNKNOWN, False)] == (OK, "")
    assert "buffer's K" in by[(FROM_BUFFER, PS_COLOR, 8, R.USER_K_UNKNOWN, True)][1]
    assert "vertex shader" in by[(FROM_GEOMETRY, PS_COLOR, 8, R.USER_K_UNKNOWN, True)][1]


def nothing_cases():
    """the table's shaders, Ks and textures for a pass without a vertex shader"""
    return [(R.FROM_NOTHING,) + c[1:] for c in ps_cases() if c[0] == FROM_GEOMETRY]


def test_pixel_shader_rule_of_a_pass_without_a_vertex_shader():
    """A list without items (include/frr.h): the id has to name a shader -- a built-in one, or a user id somebody
    registered -- and neither the K nor the texture is asked for."""
    cases = nothing_cases()
    assert len(cases) == 10 * 5 * 2
    got = R.ask(R.shader(*c) for c in cases)
    for (_, ps, K, user_K, tex), (code, text) in zip(cases, got):
        known = 0 <= ps <= PS_BLINN or (ps >= USER and user_K != R.USER_K_UNKNOWN)
        assert code == (OK if known else INVALID) and (text == "" if known else "unknown shader id" in text), (ps, K, user_K, tex, code, text)


# (use, pointer, entries, K, x1, y0, y1) -> code: a 40-wide window of 25 rows needs 1,000 entries
BUFFERS = [
    ((R.VARYINGS_OUT, 4096, 1000, 0, 40, 5, 30), OK), ((R.VARYINGS_OUT, 4096, 999, 0, 40, 5, 30), INVALID),
    ((R.VARYINGS_OUT, 0, 1000, 0, 40, 5, 30), INVALID), ((R.VARYINGS_OUT, 4098, 1000, 0, 40, 5, 30), INVALID),
    ((R.VARYINGS_OUT, 4096, 2 ** 40, 0, 32767, -32768, 32767), OK), ((R.VARYINGS_OUT, 4096, 65535 * 32767 - 1, 0, 32767, -32768, 32767), INVALID),
    ((R.COUNTS_OUT, 4096, 1, 0, 40, 5, 30), OK), ((R.COUNTS_OUT, 0, 1, 0, 40, 5, 30), INVALID), ((R.COUNTS_OUT, 4097, 1, 0, 40, 5, 30), INVALID),
    ((R.COUNTS_OUT, 0, 0, 0, 40, 5, 30), OK), ((R.COUNTS_OUT, 4097, 0, 0, 40, 5, 30), OK),      # no entries: nothing is written, any pointer
    ((R.VARYINGS_IN, 4096, 1000, 3, 40, 5, 30), OK), ((R.VARYINGS_IN, 4096, 999, 3, 40, 5, 30), INVALID),
    ((R.VARYINGS_IN, 0, 1000, 3, 40, 5, 30), INVALID), ((R.VARYINGS_IN, 4098, 1000, 3, 40, 5, 30), INVALID),
    ((R.VARYINGS_IN, 0, 1000, 0, 40, 5, 30), OK), ((R.VARYINGS_IN, 4098, 1000, 0, 40, 5, 30), INVALID),   # K = 0: NULL is fine, misaligned is not
    ((R.VARYINGS_IN, 0, 999, 0, 40, 5, 30), INVALID),
]


def test_buffer_rule_and_the_input_limit():
    got = R.ask([R.buffer(*q) for q, _ in BUFFERS] + ["c"])
    for (q, want), (code, text) in zip(BUFFERS, got):
        assert code == want and (code == OK) == (text == ""), (q, code, text)
    assert got[-1][0] == 2 ** 27     # order keys: 32 per input, in 32 bits


def test_rules_under_the_undefined_behaviour_sanitizer():
    """Every query of this module through the same program built with -fsanitize=undefined -fno-sanitize-recover=all: it
    ends clean, with the answers of the plain build.  (Host code with its own main; skipped where the host compiler has no
    UBSan runtime to link.)"""
    exe = R.build(("-fsanitize=undefined", "-fno-sanitize-recover=all"))
    if exe is None:
        pytest.skip("the host compiler's UBSan runtime is not installed")
    queries = grid_queries() + edge_queries() + [R.shader(*c) for c in ps_cases() + nothing_cases()] + [R.buffer(*q) for q, _ in BUFFERS] + ["c"]
    assert R.ask(queries, exe) == R.ask(queries)
