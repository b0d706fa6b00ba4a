"""Random whole-frame command sequences (tests/frame_model.py) on the GPU, held to the CPU frame model after every frame:
colour, depth bits, triangle ids, the statistics, every caller buffer (varyings bit for bit, counts, keep buffers) and every
host query's answer.  Each seed runs twice on fresh contexts -- with 64 bin records and 16 fan slots, so that the rungs of
the sequence overflow the work lists mid-frame and in later frames and the library cancels and replays, and with the default
lists -- and the two runs must agree byte for byte.  The mode (own targets with one or two frames in flight, caller-bound
targets), `overlap` and `clear_eager` follow from the seed.

A frame that ends with a fenced copy is read on a created stream behind frr_frame_fence only, and compared after the final
device synchronise.  frr_stats counts since frr_clear: the tiny-list run reads it at every frame end (behind the fenced
copy, which is queued by then) and holds the statistics of a fenced frame to the model like those of a read-back one -- a
half-frame that was cancelled and replayed must not count twice.  The default-list run reads it only where the frame end
synchronises anyway, so that there a fenced frame is followed by the next one with no host wait in between: its fenced
frames 0 and 1 go without statistics and without the replay counter."""
import numpy as np
import pytest

from . import frame_model as M
from . import varyings_scenes as V
from .conftest import assert_depth_equal, owned_pixel_rows
from .test_gpu_streams import _Alias

pytestmark = pytest.mark.gpu

MODES = ("own_fif1", "own_fif2", "bound")
STAT_FIELDS = ("tris_in", "tris_setup", "draws", "frag_covered", "frag_nan")
# seed -> what is known about a mismatch that is not resolved yet (pytest.mark.xfail(strict=True))
XFAIL = {}
TARGET_SENTINEL = 0x5A5A5A5A                    # what the caller-bound targets of a partitioned run hold before the first frame

_EXPECTED = {}


def _expected(oracle, seed, fixed=None, queries=False):
    """the seed's frames (queries: those of the query generator), or those of the fixed sequence frame_model.<fixed>(), with
    what the model says they leave"""
    key = fixed or (("queries", seed) if queries else seed)
    if key not in _EXPECTED:
        frames = getattr(M, fixed)() if fixed else M.generate(seed, oracle, queries=queries)
        _EXPECTED[key] = (frames, M.run_model(oracle, frames))
    return _EXPECTED[key]


def _i32(bits):
    return int(np.array([bits], np.uint32).view(np.int32)[0])


class _Run:
    """one context in the seed's mode, the caller's device buffers, and the steps of tests/frame_model.py as API calls"""

    def __init__(self, seed, tiny, part=None):
        """part: (rank, world, blocked) of a partitioned context; its caller-bound targets start as TARGET_SENTINEL"""
        import torch
        import f_renderer_amd as fr
        self.torch, self.fr = torch, fr
        self.mode, self.tiny = MODES[seed % 3], tiny
        self.st = torch.cuda.Stream()
        r = self.r = fr.Renderer(M.W, M.H, stream=self.st.cuda_stream)
        if part:
            r.set_partition(*part)
        if tiny:
            for name, value in M.TINY.items():
                r.set_option(name, value)
        r.set_option("overlap", (2, 0)[seed // 3 % 2])
        r.set_option("clear_eager", seed // 6 % 2)
        self.targets = None
        if self.mode == "bound":
            if part:
                self.targets = tuple(torch.full((M.H, M.W), _i32(TARGET_SENTINEL), dtype=torch.int32, device="cuda") for _ in range(3))
            else:
                self.targets = tuple(torch.zeros((M.H, M.W), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32))
            r.bind_targets(*(t.data_ptr() for t in self.targets))
        else:
            r.set_option("frames_in_flight", 1 if self.mode == "own_fif1" else 2)
        self.bufs = {}
        for name in M.buffer_names():
            k = M.buffer_k(name)
            self.bufs[name] = torch.full((M.ENTRIES, k) if k else (M.COUNT_CAP,), _i32(M.SENTINEL_BITS), dtype=torch.int32, device="cuda")
        self.masks = {name: torch.from_numpy(m.view(np.int32).copy()).to("cuda") for name, m in M.MASKS.items()}
        torch.cuda.synchronize()
        for slot in (0, 1):
            r.set_texture(slot, M.TEXTURES[slot])
        self.state = dict(cam=0, light=0, flat=0, slot=0)
        self._set_uniforms()
        self.meshes, self.lists, self.insts, self.tables = {}, {}, {}, {}
        self.lines = [r.upload_lines(xy, c) for xy, c in M.LINES]
        for vs in M.VS_PS:
            for name in M.MESHES:
                self.mesh(name, vs)
        self.window = M.FULL

    def _set_uniforms(self):
        s = self.state
        self.r.set_uniforms(texture_slot=s["slot"], **M.uniform_kw(self.fr, s["cam"], s["light"], s["flat"]))

    def mesh(self, name, vs):
        if (name, vs) not in self.meshes:
            vs_id = getattr(self.fr, "VS_" + vs)
            self.meshes[name, vs] = self.r.upload_mesh_indexed(*M.INDEXED[name], vs_id) if name in M.INDEXED else \
                self.r.upload_mesh(M.MESHES[name], vs_id)
        return self.meshes[name, vs]

    def table(self, name):
        """a material table of the model: uploaded, or (DEVICE_BOUND_TABLE) bound in device memory"""
        if name not in self.tables:
            if name == M.DEVICE_BOUND_TABLE:
                dev = self.torch.from_numpy(M.MATERIALS[name].view(np.uint8).copy()).to("cuda")
                self.torch.cuda.synchronize()
                assert dev.data_ptr() % 16 == 0
                self.tables[name] = self.r.bind_materials_device(dev.data_ptr(), len(M.MATERIALS[name]), keepalive=dev)
            else:
                self.tables[name] = self.r.upload_materials(M.MATERIALS[name])
        return self.tables[name]

    def ranges(self):
        x0, x1, y0, y1 = self.window
        return dict(width_range=(x0, x1), height_range=(y0, y1))

    def draw_list(self, vs, items):
        key = (vs, tuple(tuple(i) for i in items))
        if key not in self.lists:
            self.lists[key] = self.r.upload_draw_list([self.mesh(name, vs) for name, _ in items], M.MODELS[[mi for _, mi in items]].reshape(-1, 16))
        return self.lists[key]

    def prepare(self, frames):
        """set-up before the frames start, like the mesh uploads: every list that becomes the subject of a box query gets its
        bounds table once (frr_drawlist_bounds is a synchronisation point)"""
        done = set()
        for s in M.steps_of(frames):
            if s["op"] in ("boxes", "boxes_host", "bounds"):
                dl = self.draw_list(s["vs"], s["items"])
                if id(dl) not in done:
                    self.r.list_bounds(dl)
                    done.add(id(dl))

    def geometry(self, s, ps=None):
        """the geometry* call of a split pass (ps None) or the draw* call of a fused one"""
        r, fr, kind, vs, items = self.r, self.fr, s["kind"], s["vs"], s["items"]
        win = self.ranges() if ps is not None else {}
        if kind in ("plain", "indexed"):
            (name, mi), = items
            r.set_uniforms(model=M.MODELS[mi])
            return r.draw(self.mesh(name, vs), ps, **win) if ps is not None else r.geometry_processing(self.mesh(name, vs))
        if kind == "instanced":
            key = tuple(mi for _, mi in items)
            if key not in self.insts:
                self.insts[key] = r.upload_instances(M.MODELS[list(key)])
            mesh, inst = self.mesh(items[0][0], vs), self.insts[key]
            return r.draw_instanced(mesh, inst, ps, **win) if ps is not None else r.geometry_processing_instanced(mesh, inst)
        dl = self.draw_list(vs, items)
        if kind == "list":
            return r.draw_list(dl, ps, **win) if ps is not None else r.geometry_list(dl)
        keep = (self.bufs[s["keep"]] if s["keep"] in self.bufs else self.masks[s["keep"]]).data_ptr()
        if ps is not None:
            return r.draw_list_if(dl, keep, s["keep_entries"], ps, min_value=s["min"], **win)
        return r.geometry_list_if(dl, keep, s["keep_entries"], min_value=s["min"])

    def step(self, s):
        """issue one step; returns a host query's answer"""
        r, fr, op = self.r, self.fr, s["op"]
        if op == "clear":
            self.window = tuple(s["window"])
            r.clear(*M.CLEAR)
        elif op == "set_cull":
            r.set_cull(s["mode"])
        elif op == "set_uniforms":
            self.state = {k: s[k] for k in ("cam", "light", "flat", "slot")}
            self._set_uniforms()
        elif op == "set_texture":
            r.set_texture(s["slot"], M.TEXTURES[s["image"]])
        elif op == "geom":
            self.geometry(s)
        elif op == "draw":
            self.geometry(s, getattr(fr, "PS_" + s["ps"]))
        elif op == "raster":
            x0, x1, y0, y1 = self.window
            r.rasterization((x0, x1), (y0, y1), getattr(fr, "PS_" + s["ps"]))
        elif op == "lines":
            r.draw_lines(self.lines[s["list"]])
        elif op == "wireframe":
            r.draw_wireframe(M.WIRE_COLORS[s["color"]])
        elif op == "resolve":
            r.resolve_varyings(self.bufs[s["buf"]].data_ptr(), M.ENTRIES, **self.ranges())
        elif op == "shade":
            r.shade_varyings(getattr(fr, "PS_" + s["ps"]), self.bufs[s["buf"]].data_ptr(), entries=M.ENTRIES, K=M.buffer_k(s["buf"]),
                             ids=s["ids"], **self.ranges())
        elif op == "shade_items":
            r.shade_items(getattr(fr, "PS_" + s["ps"]), self.bufs[s["buf"]].data_ptr(), self.table(s["table"]), entries=M.ENTRIES,
                          K=M.buffer_k(s["buf"]), **self.ranges())
        elif op == "count":
            r.visible_pixels(s["unit"], out_ptr=self.bufs[s["buf"]].data_ptr(), entries=s["entries"], **self.ranges())
        elif op == "query":
            r.query_pixels(s["unit"], self.window, out_ptr=self.bufs[s["buf"]].data_ptr(), entries=s["entries"])
        elif op == "query_host":
            return dict(out=r.query_pixels(s["unit"], self.window, entries=s["entries"]))
        elif op == "boxes":
            r.query_boxes(self.draw_list(s["vs"], s["items"]), out_ptr=self.bufs[s["buf"]].data_ptr(), entries=s["entries"], window=self.window)
        elif op == "boxes_host":
            return dict(out=r.query_boxes(self.draw_list(s["vs"], s["items"]), entries=s["entries"], window=self.window))
        elif op == "bounds":
            lo_hi, flags = r.list_bounds(self.draw_list(s["vs"], s["items"]))
            return dict(lo_hi=lo_hi, flags=flags)
        elif op == "item_ranges":
            first, count = r.item_ranges()
            return dict(first=first, count=count)
        elif op == "setup_triangles":
            t = r.setup_triangles()
            return dict(spi=t["spi"], spf=t["spf"], rhw=t["rhw"])
        elif op == "stats":
            return r.stats()
        elif op == "sync":
            r.sync()
        else:
            raise KeyError(op)

    def end_readback(self):
        """frr_readback, then the buffers (everything has drained) and the statistics"""
        c, d, t = self.r.readback()
        st = self.r.stats()
        return dict(color=c, depth=d, tri_id=t, stats=st, bufs={k: v.cpu().numpy().view(np.uint32) for k, v in self.bufs.items()})

    def end_fenced(self):
        """the frame's targets and the buffers copied on the created stream behind frr_frame_fence: no host wait"""
        torch, st = self.torch, self.st
        self.r.frame_fence(st.cuda_stream)
        ptrs = None if self.targets else self.r.target_ptrs()
        with torch.cuda.stream(st):
            if self.targets:
                tg = tuple(x.clone() for x in self.targets)
            else:
                tg = tuple(torch.as_tensor(_Alias(p, (M.H, M.W), ts), device="cuda").clone() for p, ts in zip(ptrs, ("<i4", "<f4", "<i4")))
            return dict(targets=tg, bufs={k: v.clone() for k, v in self.bufs.items()})

    @staticmethod
    def fenced_as_host(f):
        c, d, t = (x.cpu().numpy() for x in f["targets"])
        return dict(color=c.view(np.uint8).reshape(M.H, M.W, 4), depth=d.view(np.float32).ravel(), tri_id=t.view(np.uint32).ravel(), stats=None,
                    bufs={k: v.cpu().numpy().view(np.uint32) for k, v in f["bufs"].items()})

    def close(self):
        self.torch.cuda.synchronize()
        self.r.close()


def _same_answer(op, got, want, what):
    if op == "stats":
        assert {k: got[k] for k in STAT_FIELDS} == want, f"{what}: stats {got} != {want}"
    elif op == "item_ranges":
        for k in ("first", "count"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: item_ranges {k}")
    elif op == "setup_triangles":
        np.testing.assert_array_equal(got["spi"], want["spi"], err_msg=f"{what}: setup spi")
        V.assert_bits_equal(got["spf"], want["spf"], err_msg=f"{what}: setup spf")
        V.assert_bits_equal(got["rhw"], want["rhw"], err_msg=f"{what}: setup rhw")
    elif op in ("query_host", "boxes_host"):
        np.testing.assert_array_equal(got["out"], want["out"], err_msg=f"{what}: {op}")
    elif op == "bounds":
        np.testing.assert_array_equal(got["lo_hi"].view(np.uint32), want["lo_hi"].view(np.uint32), err_msg=f"{what}: bounds lo, hi (bits)")
        np.testing.assert_array_equal(got["flags"], want["flags"], err_msg=f"{what}: bounds flags")


def _same_frame(got, want, what):
    """the first output that differs is named: ids, depth, colour, statistics, then the buffers"""
    np.testing.assert_array_equal(got["tri_id"].ravel(), want["tri_id"], err_msg=f"{what}: triangle ids")
    assert_depth_equal(got["depth"], want["depth"], err_msg=f"{what}: depth bits")
    np.testing.assert_array_equal(got["color"], want["color"], err_msg=f"{what}: colour")
    if got["stats"] is not None:
        assert {k: got["stats"][k] for k in STAT_FIELDS} == want["stats"], f"{what}: stats {got['stats']} != {want['stats']}"
    for name, b in got["bufs"].items():
        if M.buffer_k(name):
            V.assert_bits_equal(b.view(np.float32), want["bufs"][name].view(np.float32), err_msg=f"{what}: varyings buffer {name}")
        else:
            np.testing.assert_array_equal(b, want["bufs"][name], err_msg=f"{what}: count buffer {name}")


def _run(oracle, seed, tiny, fixed=None, queries=False):
    """one run of the seed's sequence (or of a fixed one under the seed's mode and options); returns (what every frame left, as
    host arrays; the replay counter at the frame ends that synchronise: {frame: count})"""
    frames, want = _expected(oracle, seed, fixed, queries)
    x = _Run(seed, tiny)
    log = [f"{fixed or 'seed'} {seed} mode={x.mode} lists={'tiny' if tiny else 'default'}"]
    got, replays, pending, fenced_stats = [None] * len(frames), {}, [], {}
    open_geom = False                           # the latest geometry pass is open or abandoned (see _Ranks.step)
    try:
        x.prepare(frames)
        for fi, steps in enumerate(frames):
            answers = iter(want[fi]["answers"])
            for s in steps[:-1]:
                log.append(f"  frame {fi}: " + M.describe(s))
                a = x.step(s)
                open_geom = _open_after(s, open_geom)
                if s["op"] in M.QUERIES:
                    op, w = next(answers)
                    assert op == s["op"]
                    _same_answer(op, a, w, f"frame {fi}, {op}")
            log.append(f"  frame {fi}: " + steps[-1]["op"])
            if steps[-1]["op"] == "readback":
                got[fi] = x.end_readback()
                replays[fi] = got[fi]["stats"]["replays"]
                _same_frame(got[fi], want[fi], f"frame {fi} (read back)")
            else:
                if open_geom:                   # (include/frr.h, frr_frame_fence: "A caller that fences such a frame calls frr_sync first.")
                    x.r.sync()
                pending.append((fi, x.end_fenced()))
                if tiny:
                    # the counters restart at the next frr_clear: a half-frame that was cancelled and replayed must not
                    # have counted twice, and this is the only place where that shows for this frame
                    fenced_stats[fi] = x.r.stats()
                    replays[fi] = fenced_stats[fi]["replays"]
        x.torch.cuda.synchronize()
        fenced_stats[len(frames) - 1] = x.r.stats()
        replays[len(frames) - 1] = fenced_stats[len(frames) - 1]["replays"]
        for fi, f in pending:
            got[fi] = x.fenced_as_host(f)
            got[fi]["stats"] = fenced_stats.get(fi)
            _same_frame(got[fi], want[fi], f"frame {fi} (fenced copy)")
        for name, mask in x.masks.items():
            np.testing.assert_array_equal(mask.cpu().numpy().view(np.uint32), M.MASKS[name], err_msg=f"the uploaded keep mask {name} changed")
        # replays: none with the default lists; with the tiny ones at least one in every frame in which the model says a rung
        # is crossed
        if not tiny:
            assert not any(replays.values()), f"replays with the default lists: {replays}"
        else:
            for fi in range(len(frames)):
                assert replays[fi] > 0 or not want[fi]["crossed"], f"frame {fi} crosses a rung, and stats() reports no replay: {replays}"
    except AssertionError as e:
        raise AssertionError("\n".join(log) + f"\n{e}") from None
    finally:
        x.close()
    return got, replays


@pytest.mark.parametrize("seed", [pytest.param(s, marks=pytest.mark.xfail(strict=True, reason=XFAIL[s])) if s in XFAIL else s for s in M.SEEDS])
def test_frame_model(oracle, seed):
    _both_runs(oracle, seed)


def _open_after(s, open_geom):
    """is the latest geometry pass open or abandoned behind step s?  include/frr.h, frr_frame_fence: "What is not whole at a
    fence: commands issued behind a frr_geometry* that no frr_raster has followed yet (an open or abandoned pass)" -- so a
    geometry* opens, and a raster, a fused draw* and the next frame's clear close; frr_query_pixels: "It closes an open pass in
    the sense of the frr_frame_fence comment" (it bins, and is verified inside the call); its host form and every other host
    query are synchronisation points, at which the commands behind the open pass were replayed, but the pass stays open for
    the commands that follow"""
    if s["op"] == "geom":
        return True
    if s["op"] in ("raster", "draw", "clear", "query"):
        return False
    return open_geom


def _both_runs(oracle, seed, fixed=None, queries=False):
    tiny, replays = _run(oracle, seed, True, fixed, queries)
    default, _ = _run(oracle, seed, False, fixed, queries)
    print(f"{fixed or 'seed'} {seed}: replays with the tiny lists, per frame: {[replays[k] for k in sorted(replays)]}")
    for fi, (a, b) in enumerate(zip(tiny, default)):
        for k in ("color", "depth", "tri_id"):
            assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), f"seed {seed} frame {fi}: {k} differs between the two runs"
        for name in a["bufs"]:
            assert a["bufs"][name].tobytes() == b["bufs"][name].tobytes(), f"seed {seed} frame {fi}: buffer {name} differs between the two runs"


@pytest.mark.parametrize("seed", [pytest.param(s, marks=pytest.mark.xfail(strict=True, reason=XFAIL[s])) if s in XFAIL else s for s in M.QSEEDS])
def test_frame_model_queries(oracle, seed):
    """The query sequences (generate(seed, queries=True)): frr_query_pixels and frr_query_boxes among every other command --
    between a geometry* and its raster, behind abandoned passes, as the command that first overflows the tiny lists, first
    behind the clear, behind camera changes, in both windows with frames in flight -- their host forms, frr_drawlist_bounds,
    and the frr_draw_list_if passes their buffers decide, within a frame and across a frame boundary, with no host wait.  Held
    to the model like the first seed set: targets, statistics (a query adds nothing but `replays`), every buffer, every
    answer; the tiny-list and the default-list run byte for byte; no replay with the default lists, at least one in a frame
    where the model says a rung is crossed."""
    _both_runs(oracle, seed, queries=True)


@pytest.mark.parametrize("seed", (0, 1, 2, 3, 7, 11))
def test_a_query_inside_a_rungs_split_pass_is_what_overflows(oracle, seed):
    """frame_model.query_overflows_a_rung in the three target modes, with option overlap 2 and 0 and clear_eager off and on: the
    per-item query between a rung's geometry and its raster is the first command that bins the pass; the line list in front
    of it is replayed with it, the count behind it needs no synchronisation point any more; a second query, of an abandoned
    pass, decides a frr_draw_list_if, and the frame is fenced with no host wait"""
    _both_runs(oracle, seed, "query_overflows_a_rung")


@pytest.mark.parametrize("seed", (0, 1, 2, 6, 7, 8))
def test_box_queries_behind_a_clear_a_camera_and_a_draw(oracle, seed):
    """frame_model.boxes_around_a_draw in the three target modes with clear_eager off and on: frr_query_boxes as the first command
    behind frr_clear, under two cameras, in front of and behind the occluder, inside a split pass in the sub-window while the
    previous frame is in flight, and the passes its buffers decide in the same and in the next frame"""
    _both_runs(oracle, seed, "boxes_around_a_draw")


@pytest.mark.parametrize("seed", range(3))
def test_cull_mode_travels_with_the_geometry_command(oracle, seed):
    """frame_model.cull_inside_split in the three target modes: frr_set_cull between a geometry* and its rasterization, which
    the generator never draws.  The open pass keeps the mode of its geometry call -- with the tiny lists through the replay of
    that call, issued when the next mode is already set -- and the next pass takes the new one."""
    _both_runs(oracle, seed, "cull_inside_split")


@pytest.mark.parametrize("seed", range(6))
def test_an_abandoned_pass_is_counted_before_the_next_pass_sizes_its_tables(oracle, seed):
    """frame_model.abandoned_then_larger in the three target modes, with option overlap 2 and 0: the ids of a pass of several
    geometry blocks behind an abandoned pass of one (seed 100 of the partitioned runs met ids that started at another count:
    the abandoned pass's block sums were scanned after the next pass had reallocated them)"""
    _both_runs(oracle, seed, "abandoned_then_larger")


def test_split_empty_list_takes_any_pixel_shader(oracle):
    """frr_geometry_list + frr_raster of a list without items takes every pixel shader frr_draw_list of it takes, and draws
    nothing (seed 5 above met the refusal: the shader was matched against a vertex shader the list does not have)"""
    import f_renderer_amd as fr
    r = fr.Renderer(M.W, M.H)
    r.set_texture(0, M.TEXTURES[0])
    dl = r.upload_draw_list([], np.zeros((0, 16), np.float32))
    r.clear(*M.CLEAR)
    for ps in (fr.PS_DEPTH, fr.PS_FLAT, fr.PS_COLOR, fr.PS_PHONG, fr.PS_BLINN):
        r.draw_list(dl, ps)
        r.geometry_list(dl)
        r.rasterization((0, M.W), (0, M.H), ps)
    c, d, t = r.readback()
    f = oracle.Frame(M.W, M.H)
    f.clear(*M.CLEAR)
    np.testing.assert_array_equal(c, f.color)
    np.testing.assert_array_equal(t, f.tri_id)
    assert_depth_equal(d, f.depth)
    st = r.stats()
    assert (st["draws"], st["tris_in"], st["tris_setup"], st["frag_covered"]) == (10, 0, 0, 0), st
    # ... and both forms refuse an id that names no shader (frr_rules.h, K_OF_NOTHING)
    for ps in (-1, fr.PS_BLINN + 1, 64 + 100000):       # (FRR_SHADER_USER_BASE + an id nobody registered)
        with pytest.raises(fr.FrrError, match="unknown shader id"):
            r.draw_list(dl, ps)
        r.geometry_list(dl)
        with pytest.raises(fr.FrrError, match="unknown shader id"):
            r.rasterization((0, M.W), (0, M.H), ps)
    r.close()


# ---- partitioned contexts ----------------------------------------------------------------------------------------------------

def _rows_mask(bands, n):
    m = np.zeros(n, bool)
    for a, b in bands:
        m[a:b] = True
    return m


class _Ranks:
    """The ranks of one partition as contexts in one process on one device, driven in lockstep: every step goes to every rank
    before the next one.  Each rank has its own targets and its own caller buffers; the one exchange between them is the
    all-reduce of a count buffer behind every frr_visible_pixels, frr_query_pixels and frr_query_boxes, which is what a
    multi-GPU caller does before it feeds the buffer to frr_draw_list_if."""

    def __init__(self, seed, world, blocked, tiny):
        import torch
        self.torch, self.world, self.blocked = torch, world, bool(blocked)
        self.x = [_Run(seed, tiny, part=(rank, world, bool(blocked))) for rank in range(world)]
        self.st = torch.cuda.Stream()           # the stream of the all-reduce
        self.reduced = False                    # an all-reduce may still be running
        self.open_geom = False                  # the latest geometry pass of the frame is not rastered (yet)

    def owners(self, window):
        """(bool [world, H]: the plane rows of the colour target each rank owns -- lines by the context's tile rows, draws and
        shades by the window's, which are the same rows here --, bool [world, y1 - y0]: the window-local rows), from the live
        contexts and checked against the rule the other partition tests stitch by"""
        x0, x1, y0, y1 = window
        plane = np.stack([_rows_mask(x.r.owned_rows((0, M.H)), M.H) for x in self.x])
        local = np.stack([_rows_mask(x.r.owned_rows((y0, y1)), y1 - y0) for x in self.x])
        for rank in range(self.world):
            np.testing.assert_array_equal(plane[rank], owned_pixel_rows(M.H, rank, self.world, self.blocked))
            np.testing.assert_array_equal(local[rank], owned_pixel_rows(y1 - y0, rank, self.world, self.blocked))
        assert (plane.sum(axis=0) == 1).all() and (local.sum(axis=0) == 1).all(), "every row has one owner"
        np.testing.assert_array_equal(plane[:, :y1 - y0], local, err_msg="a window whose tile rows are not the context's")
        return plane, local

    def step(self, s):
        """one step on every rank; returns the ranks' answers"""
        if s["op"] in ("count", "query", "boxes"):
            self.settle()                       # (frr_visible_pixels waits for no frr_frame_wait: it writes no target; nor do the queries)
        out = [x.step(s) for x in self.x]
        self.open_geom = _open_after(s, self.open_geom)
        if s["op"] in ("count", "query"):
            self.all_reduce(s["buf"], s["entries"])
        elif s["op"] == "boxes":
            # each rank's own answer is kept for the comparison with the rule under its rows; then the same sum: it is zero
            # exactly where the unpartitioned answer is, which is all a frr_draw_list_if under min_value 1 reads
            return self.all_reduce(s["buf"], s["entries"], keep=True)
        return out

    def all_reduce(self, name, entries, keep=False):
        """the ranks' counts summed on the device and written back into every rank's buffer: behind each rank's command
        (frr_frame_fence), in front of its next one (frr_frame_wait).  A count behind a geometry pass that is not rastered yet
        is guaranteed only once a synchronisation point has passed (a work list may have been too small: the count wrote
        nothing and is replayed), so there every rank synchronises first."""
        torch = self.torch
        for x in self.x:
            if self.open_geom:
                x.r.sync()
            x.r.frame_fence(self.st.cuda_stream)
        with torch.cuda.stream(self.st):
            own = [x.bufs[name][:entries].clone() for x in self.x] if keep else None
            total = torch.stack([x.bufs[name][:entries] for x in self.x]).sum(dim=0, dtype=torch.int32)
            for x in self.x:
                x.bufs[name][:entries].copy_(total)
        for x in self.x:
            x.r.frame_wait(self.st.cuda_stream)
        self.reduced = True
        return own

    def settle(self):
        """the host waits for an all-reduce that may still be running (before the buffers are copied at a frame's end)"""
        if self.reduced:
            self.st.synchronize()
            self.reduced = False

    def close(self):
        self.torch.cuda.synchronize()
        for x in self.x:
            x.r.close()


def _sum_stats(got, want, what):
    """tris_in, draws and tris_setup are every rank's (geometry is replicated); frag_covered and frag_nan are counted by the
    tile kernels of the tiles a rank owns, so the ranks' sums are the unpartitioned figures"""
    for rank, g in enumerate(got):
        assert {k: g[k] for k in ("tris_in", "tris_setup", "draws")} == {k: want[k] for k in ("tris_in", "tris_setup", "draws")}, f"{what}, rank {rank}: {g} != {want}"
    for k in ("frag_covered", "frag_nan"):
        assert sum(g[k] for g in got) == want[k], f"{what}: the ranks' {k} {[g[k] for g in got]} do not add up to {want[k]}"


def _entries_of(local_rows, window):
    """bool [W * H]: the depth / id entries i of a window whose window-local row i // x1 is one of `local_rows`"""
    x0, x1, y0, y1 = window
    row = np.arange(M.W * M.H) // x1
    out = np.zeros(M.W * M.H, bool)
    out[row < y1 - y0] = local_rows[row[row < y1 - y0]]
    return out


def _stitch_frame(got, want, window, plane, local, bound, what, ever=None):
    """ids, depth bits and colour of the ranks stitched by the owner of each row -- colour by its plane row, depth and ids by
    the window-local row i // x1 of the entry -- equal the unpartitioned model's; the rows and entries a rank does not own
    hold the clear values in the context's own targets and, in caller-bound ones, those or TARGET_SENTINEL.  (ever[rank]:
    the entries the rank owns under ANY window of the run.  The depth stride is the window's x1, so an entry of another rank
    in this frame may be the rank's own in a frame with another window: a caller-bound target, which nobody brings up to
    date, may still hold that frame's fragment there.)"""
    x0, x1, y0, y1 = window
    world = len(got)
    row = np.arange(M.W * M.H) // x1
    inside = row < y1 - y0
    color = np.zeros((M.H, M.W, 4), np.uint8)
    depth, ids = np.zeros(M.W * M.H, np.float32), np.zeros(M.W * M.H, np.uint32)
    clear_rgba = np.array(M.CLEAR[0], np.uint8)
    clear_bits, sentinel = np.array([M.CLEAR[1]], np.float32).view(np.uint32)[0], np.uint32(TARGET_SENTINEL)
    for rank, g in enumerate(got):
        mine = np.zeros(M.W * M.H, bool)
        mine[inside] = local[rank][row[inside]]
        color[plane[rank]] = g["color"][plane[rank]]
        depth[mine], ids[mine] = g["depth"][mine], g["tri_id"].ravel()[mine]
        other_c = g["color"][~plane[rank]].reshape(-1, 4)
        never = ~(mine | ever[rank]) if bound and ever is not None else ~mine
        other_d, other_t = g["depth"].view(np.uint32)[never], g["tri_id"].ravel()[never]
        if bound:
            s4 = np.full(4, 0x5A, np.uint8)
            assert ((other_c == clear_rgba).all(axis=1) | (other_c == s4).all(axis=1)).all(), f"{what}, rank {rank}: colour in rows of other ranks"
            assert ((other_d == clear_bits) | (other_d == sentinel)).all(), f"{what}, rank {rank}: depth in entries of other ranks"
            assert ((other_t == M.NONE) | (other_t == sentinel)).all(), f"{what}, rank {rank}: ids in entries of other ranks"
        else:
            assert (other_c == clear_rgba).all(), f"{what}, rank {rank}: an own target's rows of other ranks are not the cleared ones"
            assert (other_d == clear_bits).all() and (other_t == M.NONE).all(), f"{what}, rank {rank}: an own target's entries of other ranks are not the cleared ones"
    nobody = ~inside
    depth[nobody], ids[nobody] = want["depth"][nobody], want["tri_id"][nobody]     # (checked above on every rank: nobody draws there)
    assert (want["depth"].view(np.uint32)[nobody] == clear_bits).all() and (want["tri_id"][nobody] == M.NONE).all()
    np.testing.assert_array_equal(ids, want["tri_id"], err_msg=f"{what}: stitched triangle ids")
    assert_depth_equal(depth, want["depth"], err_msg=f"{what}: stitched depth bits")
    np.testing.assert_array_equal(color, want["color"], err_msg=f"{what}: stitched colour")


class _Buffers:
    """The caller's varyings buffers over the frames of a run.  A buffer outlives a frame and the window changes between
    frames, so the stitched buffer is kept up from frame to frame: where the model says this frame's resolves wrote, the entry
    comes from the rank that owns its window-local row; every entry a rank never had to write keeps the sentinel there."""

    def __init__(self, world):
        self.stitched = M.new_buffers()
        self.touched = [{k: np.zeros(v.shape[0], bool) for k, v in self.stitched.items() if M.buffer_k(k)} for _ in range(world)]

    def frame(self, got, want, window, local, what, counts=None):
        """counts: the count buffers as the ranks hold them where they differ from the model's (box answers, summed)"""
        x0, x1, y0, y1 = window
        row = np.arange(M.ENTRIES) // x1
        inside = row < y1 - y0
        for name, b in want["bufs"].items():
            if not M.buffer_k(name):
                b = counts[name] if counts and name in counts else b
                for rank, g in enumerate(got):
                    np.testing.assert_array_equal(g["bufs"][name], b, err_msg=f"{what}: count buffer {name} of rank {rank}")
                continue
            wrote = want["wrote"].get(name, np.zeros(M.ENTRIES, bool))
            for rank, g in enumerate(got):
                mine = np.zeros(M.ENTRIES, bool)
                mine[inside] = local[rank][row[inside]]
                mine &= wrote
                self.touched[rank][name] |= mine
                self.stitched[name][mine] = g["bufs"][name][mine]
                rest = g["bufs"][name][~self.touched[rank][name]]
                assert (rest == M.SENTINEL_BITS).all(), f"{what}: varyings buffer {name} of rank {rank} was written outside the rows it owns"
            V.assert_bits_equal(self.stitched[name].view(np.float32), b.view(np.float32), err_msg=f"{what}: stitched varyings buffer {name}")


_EXPECTED_X = {}


def _expected_x(oracle, key):
    """the frames of an extended seed, of a query seed (key: ("queries", seed)) or of a fixed sequence of frame_model, with what
    the partitioned model says they leave"""
    if key not in _EXPECTED_X:
        frames = getattr(M, key)() if isinstance(key, str) else M.generate(key[1], oracle, queries=True) if isinstance(key, tuple) else \
            M.generate(key, oracle, extended=True)
        _EXPECTED_X[key] = (frames, M.run_model(oracle, frames, partitioned=True))
    return _EXPECTED_X[key]


def _run_partitioned(oracle, seed, world, blocked, tiny, key):
    import f_renderer_amd as fr
    frames, want = _expected_x(oracle, key)
    p = _Ranks(seed, world, blocked, tiny)
    bound = p.x[0].mode == "bound"
    log = [f"{key} world={world} blocked={blocked} mode={p.x[0].mode} lists={'tiny' if tiny else 'default'}"]
    bufs, replays, pending = _Buffers(world), {}, []
    # the ranks' count buffers where they are not the model's: behind a box query a buffer holds the SUM of the ranks' own
    # answers (include/frr.h: "The ranks' values do NOT add up to the unpartitioned ones"), until a count or a query replaces it
    box_sum = {name: np.zeros(M.COUNT_CAP, np.uint32) for name in M.buffer_names() if not M.buffer_k(name)}
    box_on = {name: np.zeros(M.COUNT_CAP, bool) for name in box_sum}
    own_answers = []                            # (what, the ranks' own device answers, the rule's under each rank's rows)
    try:
        for x in p.x:
            x.prepare(frames)
        ever = [np.zeros(M.W * M.H, bool) for _ in range(world)]
        for window in {tuple(steps[0]["window"]) for steps in frames}:
            for rank, rows in enumerate(p.owners(window)[1]):
                ever[rank] |= _entries_of(rows, window)
        for fi, steps in enumerate(frames):
            answers = iter(want[fi]["answers"])
            boxes = iter(want[fi]["boxes"])
            window = tuple(steps[0]["window"])
            rows = [M.rank_tile_rows(window, rank, world, bool(blocked)) for rank in range(world)]
            for s in steps[:-1]:
                log.append(f"  frame {fi}: " + M.describe(s))
                if s.get("refused"):
                    for rank, x in enumerate(p.x):
                        with pytest.raises(fr.FrrError) as err:
                            x.step(s)
                        assert err.value.code == fr.FRR_ERR_INVALID, f"rank {rank}: {err.value}"
                    continue
                got = p.step(s)
                if s["op"] in ("count", "query"):
                    box_on[s["buf"]][:s["entries"]] = False
                elif s["op"] == "boxes":
                    b = next(boxes)
                    assert b["buf"] == s["buf"] and b["out"].size == s["entries"]
                    mine = [M.box_answer(b["args"], rows[rank])[0] for rank in range(world)]
                    own_answers.append((f"frame {fi}, {M.describe(s)}", got, mine))
                    box_sum[s["buf"]][:s["entries"]] = np.sum(mine, axis=0, dtype=np.uint64).astype(np.uint32)
                    box_on[s["buf"]][:s["entries"]] = True
                if s["op"] in M.QUERIES:
                    op, w = next(answers)
                    assert op == s["op"]
                    if op == "stats":
                        _sum_stats(got, w, f"frame {fi}, stats")
                    elif op == "query_host":    # (the ranks' counts add up to the unpartitioned ones)
                        np.testing.assert_array_equal(np.sum([a["out"] for a in got], axis=0, dtype=np.uint64), w["out"], err_msg=f"frame {fi}, query_host: the ranks' sum")
                    elif op == "boxes_host":    # (a rank's answer is its own: the rule under the rows it owns)
                        for rank, a in enumerate(got):
                            np.testing.assert_array_equal(a["out"], M.box_answer(w["args"], rows[rank])[0], err_msg=f"frame {fi}, boxes_host, rank {rank}")
                    else:
                        for rank, a in enumerate(got):
                            _same_answer(op, a, w, f"frame {fi}, {op}, rank {rank}")
            log.append(f"  frame {fi}: " + steps[-1]["op"])
            plane, local = p.owners(window)
            for rank in range(world):
                np.testing.assert_array_equal(np.repeat(rows[rank], 32)[:window[3] - window[2]], local[rank], err_msg="the tile rows the rule is asked under")
            p.settle()
            counts = {name: np.where(box_on[name], box_sum[name], want[fi]["bufs"][name]) for name in box_sum if box_on[name].any()}
            if steps[-1]["op"] == "readback":
                got = [x.end_readback() for x in p.x]
                replays[fi] = [g["stats"]["replays"] for g in got]
                pending.append((fi, window, plane, local, got, None, counts))
            else:
                # (include/frr.h: what is issued behind a frr_geometry* that no frr_raster has followed is guaranteed only once a
                # synchronisation point has passed -- frr_frame_fence is none, and seed 109 met it: with the tiny lists an
                # abandoned rung cancelled the shade behind it, and the fenced copy was taken before the replay)
                if p.open_geom:
                    for x in p.x:
                        x.r.sync()
                pending.append((fi, window, plane, local, None, [x.end_fenced() for x in p.x], counts))
                if tiny:
                    pending[-1] += ([x.r.stats() for x in p.x],)
                    replays[fi] = [st["replays"] for st in pending[-1][7]]
        p.torch.cuda.synchronize()
        last = [x.r.stats() for x in p.x]
        replays[len(frames) - 1] = [st["replays"] for st in last]
        # (the frames are compared in their order: a varyings buffer carries what earlier frames wrote)
        for what, got, mine in own_answers:
            for rank, (g, w) in enumerate(zip(got, mine)):
                np.testing.assert_array_equal(g.cpu().numpy().view(np.uint32), w, err_msg=f"{what}: rank {rank}'s own answer")
        for fi, window, plane, local, got, fenced, counts, *stats in pending:
            if got is None:
                got = [_Run.fenced_as_host(f) for f in fenced]
                for rank, g in enumerate(got):
                    g["stats"] = stats[0][rank] if stats else last[rank] if fi == len(frames) - 1 else None
            _check_partitioned_frame(got, want[fi], window, plane, local, bound, bufs, f"frame {fi} ({'fenced copy' if fenced else 'read back'})", ever, counts)
        for x in p.x:
            for name, mask in x.masks.items():
                np.testing.assert_array_equal(mask.cpu().numpy().view(np.uint32), M.MASKS[name], err_msg=f"the uploaded keep mask {name} changed")
        # replays: none with the default lists; with the tiny ones on EVERY rank in a frame where the model says a geometry*
        # call crosses a rung of the fan slots (frr_geometry* never filters: the need is the unpartitioned one).  A rank's need
        # of bin records, and of fan slots under a fused draw*, which filters its inputs by the rank's rows, is a fraction the
        # model does not compute: a rank that owns nothing needs none.
        if not tiny:
            assert not any(any(v) for v in replays.values()), f"replays with the default lists: {replays}"
        else:
            for fi in range(len(frames)):
                assert all(n > 0 for n in replays[fi]) or not want[fi]["crossed_fan"], f"frame {fi} crosses a rung of the fan slots: replays per rank {replays}"
    except AssertionError as e:
        raise AssertionError("\n".join(log) + f"\n{e}") from None
    finally:
        p.close()
    return replays


def _check_partitioned_frame(got, want, window, plane, local, bound, bufs, what, ever=None, counts=None):
    _stitch_frame(got, want, window, plane, local, bound, what, ever)
    if got[0]["stats"] is not None:
        _sum_stats([g["stats"] for g in got], want["stats"], what)
    bufs.frame(got, want, window, local, what, counts)


def _partition_of(seed):
    return (2, 3, 4)[seed % 3], seed // 3 % 2, seed % 2 == 1


@pytest.mark.parametrize("seed", [pytest.param(s, marks=pytest.mark.xfail(strict=True, reason=XFAIL[s])) if s in XFAIL else s for s in M.XSEEDS])
def test_frame_model_partitioned(oracle, seed):
    """The extended sequences (frr_shade_items, passes rastered again, abandoned passes) on the ranks of a partition, in
    lockstep, held to the UNPARTITIONED model after every frame.  The seed decides the world (2, 3 or 4 ranks: the frame and
    the 80-row window both have three tile rows, so in a world of 4 one rank owns nothing), the layout, the target mode and the
    work lists (tiny on odd seeds, default on even ones).  Compared: colour, depth bits and ids stitched by the owner of each
    row; the varyings buffers stitched the same way, entries no rank had to write still the sentinel; count buffers (all-
    reduced), keep masks and host queries equal to the model's on every rank; tris_in, draws and tris_setup on every rank,
    frag_covered and frag_nan as the ranks' sum; replays.
    Rows of other ranks.  include/frr.h (frr_bind_targets): "only the tile rows the rank owns are defined in caller-owned
    targets ...; the ctx's own targets are brought up to date in full whenever they are read back".  For own targets that is
    asserted as it is implemented (k_clear_unowned_rows, unowned_debt in frr_api.hip): at a read-back or behind frr_target_ptrs
    every row and entry of another rank holds the frame's clear values.  Caller-bound targets were filled with TARGET_SENTINEL
    before the first frame: a rank never draws there, but a clear that is not performed inside a full-window draw (a sub-
    window, a command other than a draw first, option clear_eager) clears the whole target, so such rows hold the sentinel or
    the clear values and nothing else -- of depth and ids, the entries that are the rank's own under no window of the run: the
    depth stride is the window's x1, and an entry of another rank in this frame may hold the rank's own fragment of a frame
    with the other window, which nobody clears in a caller-bound target.
    Seed 100 found the abandoned pass whose block sums were scanned after the next pass had reallocated them:
    test_an_abandoned_pass_is_counted_before_the_next_pass_sizes_its_tables."""
    world, blocked, tiny = _partition_of(seed)
    replays = _run_partitioned(oracle, seed, world, blocked, tiny, seed)
    print(f"seed {seed}: world {world}, replays per frame and rank: {replays}")


@pytest.mark.parametrize("seed", [pytest.param(s, marks=pytest.mark.xfail(strict=True, reason=XFAIL[s])) if s in XFAIL else s for s in M.QSEEDS])
def test_frame_model_queries_partitioned(oracle, seed):
    """The query sequences on the ranks of a partition, held to the unpartitioned model like the extended ones.  Behind a
    frr_query_pixels the count buffer is all-reduced as behind a frr_visible_pixels: the ranks' counts add up to the model's.
    Behind a frr_query_boxes every rank's own answer is first held to the rule under the tile rows that rank owns
    (frame_model.box_answer with row_owned), then the buffer is all-reduced by the same sum: the ranks' answers do not add up to
    the unpartitioned one, but the sum is zero exactly where it is (tests/test_frame_model_cpu.py holds that for these very
    queries), so a frr_draw_list_if under min_value 1 -- the only one the generator feeds with box answers -- keeps the model's
    items on every rank and the stitched frame is the model's.  At a frame's end such a buffer is compared with the sum of the
    rule's per-rank answers."""
    world, blocked, tiny = _partition_of(seed)
    replays = _run_partitioned(oracle, seed, world, blocked, tiny, ("queries", seed))
    print(f"seed {seed}: world {world}, replays per frame and rank: {replays}")


@pytest.mark.parametrize("fixed", ["query_overflows_a_rung", "boxes_around_a_draw"])
@pytest.mark.parametrize("seed", range(3))
def test_the_fixed_query_sequences_on_every_rank(oracle, seed, fixed):
    """the two fixed query sequences in worlds of 2, 3 and 4 ranks (tiny lists in the world of 3)"""
    world, blocked, tiny = _partition_of(seed)
    _run_partitioned(oracle, seed, world, blocked, tiny, fixed)


@pytest.mark.parametrize("seed", range(3))
def test_refused_behind_a_fused_pass_on_every_rank(oracle, seed):
    """frame_model.refused_behind_fused in worlds of 2, 3 and 4 ranks: frr_draw_wireframe, frr_readback_setup,
    frr_geometry_item_ranges, frr_resolve_varyings, frr_visible_pixels and frr_shade_items behind a fused frr_draw_list answer
    FRR_ERR_INVALID on every rank, and the frame is the one the other steps leave"""
    world, blocked, tiny = _partition_of(seed)
    _run_partitioned(oracle, seed, world, blocked, tiny, "refused_behind_fused")


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_lines_take_the_contexts_tile_rows_in_a_short_window(oracle, world, blocked):
    """frame_model.line_ownership: a pass, a line list over it and a shade in a window of 40 rows -- two tile rows, where the
    context has three.  frr_draw_lines takes its owner from the context's tile rows, the others from the window's.
    Every rank's colour is the model's frame with each command undone outside the rows that command owns on the rank
    (frame_model.run_rank); the context's own targets hold the clear colour in every other row at the read-back.
    Interleaved the two rules agree, and the ranks stitch to the unpartitioned frame.  Blocked they do not: with two ranks
    plane rows 32 .. 39 are the draws' on rank 1 and the lines' on rank 0, and that tile row is complete on no rank
    (include/frr.h, frr_draw_lines: the limit of the rule)."""
    frames = M.line_ownership()
    want, = M.run_model(oracle, frames)
    stitched = np.zeros_like(want["color"])
    for rank in range(world):
        x = _Run(0, False, part=(rank, world, blocked))
        try:
            for s in frames[0][:-1]:
                x.step(s)
            got = x.end_readback()
        finally:
            x.close()
        mine = M.run_rank(oracle, frames[0], rank, world, blocked)
        np.testing.assert_array_equal(got["color"], mine["color"], err_msg=f"rank {rank}: colour")
        np.testing.assert_array_equal(got["tri_id"], mine["tri_id"], err_msg=f"rank {rank}: triangle ids")
        assert_depth_equal(got["depth"], mine["depth"], err_msg=f"rank {rank}: depth bits")
        rows = M.command_rows("lines", M.LINE_WINDOW, M.H, rank, world, blocked)
        np.testing.assert_array_equal(rows, owned_pixel_rows(M.H, rank, world, blocked))
        stitched[rows] = got["color"][rows]
    if not blocked:
        np.testing.assert_array_equal(stitched, want["color"], err_msg="the ranks' images stitched by plane row")
    elif world == 2:
        assert (stitched[32:40] != want["color"][32:40]).any() and (stitched[:32] == want["color"][:32]).all()
