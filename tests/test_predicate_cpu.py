"""CPU: the keep rule of predicated list passes (frr_rules.h: item_kept, keep_rule), compiled with the host compiler and asked
through tests/keep_rule.py -- the comparison against NumPy's unsigned >=, every error case of the argument rule, and the same
queries through a build under the host compiler's address and undefined-behaviour sanitizers -- and the oracle side of
tests/test_gpu_predicate.py: the expected frame of every mask it uses is held to the definition, the reference's loop over
the kept items alone, and the `hidden` scene to its condition."""
import numpy as np
import pytest

from . import keep_rule as K
from . import predicate_scenes as P
from . import drawlist_scenes as D
from .conftest import assert_depth_equal

MINS = [0, 1, 6, 0x80000000, 0xFFFFFFFF]


def kept_queries():
    out = []
    for mv in MINS:
        for v in (0, 1, (mv - 1) & 0xFFFFFFFF, mv, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
            out.append((v, mv))
    return out


def test_item_kept_is_the_unsigned_comparison():
    q = kept_queries()
    got = K.ask(K.kept(v, mv) for v, mv in q)
    want = np.array([v for v, _ in q], np.uint32) >= np.array([mv for _, mv in q], np.uint32)
    assert [g[0] for g in got] == [int(w) for w in want]
    by = dict(zip(q, (g[0] for g in got)))
    assert by[(0x80000000, 1)] == 1 and by[(0xFFFFFFFF, 6)] == 1           # not a signed comparison
    assert by[(0x7FFFFFFF, 0x80000000)] == 0 and by[(0, 0)] == 1 and by[(0xFFFFFFFE, 0xFFFFFFFF)] == 0
    assert P.kept_of([v for v, _ in q[:7]], q[0][1]).tolist() == want[:7].tolist()     # the tests' own helper is that comparison


# (pointer, keep_entries, nitems) -> code
RULES = [
    ((4096, 7, 7), K.OK), ((4096, 8, 7), K.OK), ((4096, 2 ** 40, 7), K.OK),
    ((4096, 6, 7), K.INVALID), ((4096, 0, 1), K.INVALID),                   # fewer entries than items
    ((0, 7, 7), K.INVALID), ((0, 0, 1), K.INVALID),                         # NULL with items
    ((4097, 7, 7), K.INVALID), ((4098, 7, 7), K.INVALID), ((4099, 7, 7), K.INVALID),   # not 4-byte aligned
    ((0, 0, 0), K.OK), ((0, 5, 0), K.OK), ((4096, 0, 0), K.OK),             # no items: nothing is read, NULL is fine
    ((4098, 0, 0), K.INVALID),                                              # ... a misaligned pointer never is
    ((2 ** 63 + 4, 2 ** 64 - 1, 2 ** 27), K.OK),
]


def test_keep_rule_every_error_case():
    got = K.ask(K.rule(*q) for q, _ in RULES)
    for (q, want), (code, text) in zip(RULES, got):
        assert code == want and (code == K.OK) == (text == ""), (q, code, text)
    by = {q: t for (q, _), (_, t) in zip(RULES, got)}
    assert "keep_entries" in by[(4096, 6, 7)] and "NULL" in by[(0, 7, 7)] and "aligned" in by[(4098, 7, 7)]
    assert "NULL" in by[(0, 0, 1)]                                          # the pointer is asked before the count


def test_keep_rule_under_the_address_and_undefined_behaviour_sanitizers():
    """Every query of this module through the same program -- host code with its own main -- built with
    -fsanitize=address,undefined -fno-sanitize-recover=all: it ends clean, with the answers of the plain build.  (Skipped
    where the host compiler has no sanitizer runtime to link.)"""
    exe = K.build(("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if exe is None:
        pytest.skip("the host compiler's sanitizer runtimes are not installed")
    queries = [K.kept(v, mv) for v, mv in kept_queries()] + [K.rule(*q) for q, _ in RULES]
    assert K.ask(queries, exe) == K.ask(queries)


def test_the_hidden_scene_has_hidden_and_visible_items(oracle):
    counts = P.hidden_counts(oracle)
    assert (counts == 0).sum() >= 1 and (counts > 0).sum() >= 2
    sc = P.scene("hidden")
    # the frame without the hidden items is the frame with them, in depth and colour: what feeding the counts back relies on
    full = P.expected(oracle, "hidden", np.ones(sc.nitems, bool))[0]
    seen = P.expected(oracle, "hidden", counts > 0)[0]
    assert_depth_equal(seen.depth, full.depth)
    np.testing.assert_array_equal(seen.color, full.color)


CASES = P.gpu_cases() + [("hidden", "visible", None)]


@pytest.mark.parametrize("name", sorted({c[0] for c in CASES}))
def test_expected_frames_are_the_loop_over_the_kept_items(oracle, name):
    """The predicated frame over mask m -- dropped items as empty meshes -- equals the plain oracle loop over a Scene built
    from the kept items only, in depth, RGBA8, triangle ids (dense over the survivors), the setup list and the counters; a
    dropped item emits nothing and a kept one what it emits in that loop."""
    sc = P.scene(name)
    n = 0
    for cname, label, kept in CASES:
        if cname != name:
            continue
        if kept is None:
            kept = P.hidden_counts(oracle) > 0
        f, setup, per = P.expected(oracle, name, kept)
        sub = P.kept_scene(sc, kept)
        g, gsetup, gper = D.oracle_list_loop(oracle, sub)
        assert_depth_equal(f.depth, g.depth, err_msg=f"{name} {label}: depth")
        np.testing.assert_array_equal(f.color, g.color, err_msg=f"{name} {label}: colour")
        np.testing.assert_array_equal(f.tri_id, g.tri_id, err_msg=f"{name} {label}: ids")
        assert setup.tobytes() == gsetup.tobytes()
        assert [p for p, k in zip(per, kept) if k] == gper and all(p == 0 for p, k in zip(per, kept) if not k)
        assert (f.counters.tris_setup, f.counters.frag_covered, f.counters.frag_nan) == (g.counters.tris_setup, g.counters.frag_covered, g.counters.frag_nan)
        n += 1
    assert n >= 1
