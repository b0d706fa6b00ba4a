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
from .conftest import assert_depth_equal
from .test_gpu_streams import _Alias

pytestmark = pytest.mark.gpu

MODES = ("own_fif1", "own_fif2", "bound")
STAT_FIELDS = ("tris_in", "tris_setup", "draws", "frag_covered", "frag_nan")
# seed -> what is known about a mismatch that is not resolved yet (pytest.mark.xfail(strict=True))
XFAIL = {}

_EXPECTED = {}


def _expected(oracle, seed, fixed=None):
    """the seed's frames, or those of the fixed sequence frame_model.<fixed>(), with what the model says they leave"""
    key = fixed or seed
    if key not in _EXPECTED:
        frames = getattr(M, fixed)() if fixed else M.generate(seed, oracle)
        _EXPECTED[key] = (frames, M.run_model(oracle, frames))
    return _EXPECTED[key]


def _i32(bits):
    return int(np.array([bits], np.uint32).view(np.int32)[0])


class _Run:
    """one context in the seed's mode, the caller's device buffers, and the steps of tests/frame_model.py as API calls"""

    def __init__(self, seed, tiny):
        import torch
        import f_renderer_amd as fr
        self.torch, self.fr = torch, fr
        self.mode, self.tiny = MODES[seed % 3], tiny
        self.st = torch.cuda.Stream()
        r = self.r = fr.Renderer(M.W, M.H, stream=self.st.cuda_stream)
        if tiny:
            for name, value in M.TINY.items():
                r.set_option(name, value)
        r.set_option("overlap", (2, 0)[seed // 3 % 2])
        r.set_option("clear_eager", seed // 6 % 2)
        self.targets = None
        if self.mode == "bound":
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
        self.meshes, self.lists, self.insts = {}, {}, {}
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

    def ranges(self):
        x0, x1, y0, y1 = self.window
        return dict(width_range=(x0, x1), height_range=(y0, y1))

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
        key = (vs, tuple(items))
        if key not in self.lists:
            self.lists[key] = r.upload_draw_list([self.mesh(name, vs) for name, _ in items], M.MODELS[[mi for _, mi in items]].reshape(-1, 16))
        dl = self.lists[key]
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
        elif op == "count":
            r.visible_pixels(s["unit"], out_ptr=self.bufs[s["buf"]].data_ptr(), entries=s["entries"], **self.ranges())
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


def _run(oracle, seed, tiny, fixed=None):
    """one run of the seed's sequence (or of a fixed one under the seed's mode and options); returns (what every frame left, as
    host arrays; the replay counter at the frame ends that synchronise: {frame: count})"""
    frames, want = _expected(oracle, seed, fixed)
    x = _Run(seed, tiny)
    log = [f"{fixed or 'seed'} {seed} mode={x.mode} lists={'tiny' if tiny else 'default'}"]
    got, replays, pending, fenced_stats = [None] * len(frames), {}, [], {}
    try:
        for fi, steps in enumerate(frames):
            answers = iter(want[fi]["answers"])
            for s in steps[:-1]:
                log.append(f"  frame {fi}: " + M.describe(s))
                a = x.step(s)
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


def _both_runs(oracle, seed, fixed=None):
    tiny, replays = _run(oracle, seed, True, fixed)
    default, _ = _run(oracle, seed, False, fixed)
    print(f"{fixed or 'seed'} {seed}: replays with the tiny lists, per frame: {[replays[k] for k in sorted(replays)]}")
    for fi, (a, b) in enumerate(zip(tiny, default)):
        for k in ("color", "depth", "tri_id"):
            assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), f"seed {seed} frame {fi}: {k} differs between the two runs"
        for name in a["bufs"]:
            assert a["bufs"][name].tobytes() == b["bufs"][name].tobytes(), f"seed {seed} frame {fi}: buffer {name} differs between the two runs"


@pytest.mark.parametrize("seed", range(3))
def test_cull_mode_travels_with_the_geometry_command(oracle, seed):
    """frame_model.cull_inside_split in the three target modes: frr_set_cull between a geometry* and its rasterization, which
    the generator never draws.  The open pass keeps the mode of its geometry call -- with the tiny lists through the replay of
    that call, issued when the next mode is already set -- and the next pass takes the new one."""
    _both_runs(oracle, seed, "cull_inside_split")


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
