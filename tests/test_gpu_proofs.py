"""A draw cannot fail, also for a consumer that reads its frames only in stream order (include/frr.h, FRR_ERR_CAPACITY):
frr_frame_fence + frr_target_ptrs on own targets, caller-bound targets under option bound_targets_in_flight.  The library
keeps that promise by verifying every raster pass whose DrawSig it has not seen complete (frr_ctx::proven); these tests
change what a pass reads while everything the old signature recorded stays the same -- a device-bound mesh rewritten in
place behind frr_sync, a texture re-uploaded under a user vertex shader that samples it, uniforms.texture_slot switched --
with work lists so small that the heavy scene overflows them, and read every frame through a fence only.  Also the
reverse edge, frr_frame_wait: several streams at once, and a pending clear of an earlier binding in between.

Scenes: L fits the tiny lists, H has the same triangle count and overflows them (checked on a fresh ctx in every test:
otherwise the test proves nothing).  Every frame is the oracle's, through the fence and through frr_readback."""
import numpy as np
import pytest

from .conftest import assert_depth_equal
from .test_gpu_streams import _Alias

pytestmark = pytest.mark.gpu

W, H = 352, 224
N_TRIS = 1200
CLEAR = (7, 7, 7, 7)
TINY = {"bin": ("bin_capacity", 2400), "fan": ("fan_capacity", 64)}
MODES = ["own_fif1", "own_fif2", "bound_in_flight"]

# A user vertex shader that moves vertices by what it samples: input = clip position A (4), clip position B (4), RGB (3).
# A texel of 255 (0) takes B (A), u.user[0] > 0.5 swaps the choice; the pixel shader is PS_COLOR's.  The selection is
# exact, so the frame is VS_CLIP_COLOR's of the selected positions.
_SELECT_VS = r"""
__device__ void frr_user_vs(const frr::DevUniforms &u, const float *in, float pos[4], float *ctx)
{
    float t[4];
    SAMPLE;
    const int o = ((t[0] > 0.5f) != (u.user[0] > 0.5f)) ? 4 : 0;
    pos[0] = in[o]; pos[1] = in[o + 1]; pos[2] = in[o + 2]; pos[3] = in[o + 3];
    ctx[0] = in[8]; ctx[1] = in[9]; ctx[2] = in[10];
}
__device__ void frr_user_ps(const frr::DevUniforms &u, const float *ctx, float out[4], const float *u8lut)
{
    out[0] = ctx[0]; out[1] = ctx[1]; out[2] = ctx[2]; out[3] = 1.0f;
}
"""
SELECT_SLOT0 = _SELECT_VS.replace("SAMPLE", "frr::sample_2d_slot(u, 0, 0.5f, 0.5f, t)")   # texture slot 0
SELECT_CURRENT = _SELECT_VS.replace("SAMPLE", "frr::sample_2d(u, 0.5f, 0.5f, t)")          # uniforms.texture_slot's


def _tex(v):
    return np.full((4, 4, 4), v, np.uint8)


def _tris(n, seed, r_px, ndc):
    """n clip-space triangles of radius r_px pixels, centres within +-ndc, w in [1, 4] (VS_CLIP layout)"""
    from f_renderer_amd import scenes
    u = scenes.splitmix_u01(seed, 10 * n).reshape(n, 10)
    w = 1.0 + 3.0 * u[:, 0]
    cx, cy = ndc * (2.0 * u[:, 1] - 1.0), ndc * (2.0 * u[:, 2] - 1.0)
    r = 2.0 * r_px / W
    out = np.empty((n, 3, 4), np.float64)
    for k in range(3):
        out[:, k, 0] = (cx + r * (2.0 * u[:, 3 + 2 * k] - 1.0)) * w
        out[:, k, 1] = (cy + r * (2.0 * u[:, 4 + 2 * k] - 1.0) * (W / H)) * w
        out[:, k, 2] = 0.5 * w
        out[:, k, 3] = w
    return out.astype(np.float32)


_SCENES = {}


def _scenes(oracle, kind):
    """(positions {L, H}, colours, oracle frames {L, H}) of the overflow kind ('bin': H has large triangles, 'fan': H
    straddles the frustum, L never does)"""
    if kind not in _SCENES:
        from f_renderer_amd import scenes
        pos = {"L": _tris(N_TRIS, 11, 2.0, 0.8)}
        pos["H"] = _tris(N_TRIS, 12, 48.0, 0.6) if kind == "bin" else \
            scenes.random_clip_triangles(N_TRIS, W, H, seed=13, spread=1.5, w_jitter=0.6)
        col = scenes.splitmix_u01(14, N_TRIS * 9).reshape(N_TRIS, 3, 3).astype(np.float32)
        frames = {}
        for s in "LH":
            f = oracle.Frame(W, H)
            f.clear(CLEAR, 0.0)
            f.draw(np.concatenate([pos[s], col], axis=2), oracle.VS_CLIP_COLOR, oracle.PS_COLOR, oracle.make_uniforms())
            frames[s] = f
        _SCENES[kind] = (pos, col, frames)
    return _SCENES[kind]


def _tris7(sc, s):
    return np.ascontiguousarray(np.concatenate([sc[0][s], sc[1]], axis=2))


def _tris11(sc, a, b):
    return np.ascontiguousarray(np.concatenate([sc[0][a], sc[0][b], sc[1]], axis=2))


def _tiny(r, kind):
    r.set_option(*TINY[kind])


_CHECKED = set()


def _assert_not_vacuous(oracle, kind):
    """On a fresh ctx with the same tiny lists: L alone fits, H alone overflows (the draw replays)"""
    import f_renderer_amd as fr
    if kind in _CHECKED:
        return
    sc = _scenes(oracle, kind)
    for s, want in (("L", False), ("H", True)):
        r = fr.Renderer(W, H)
        _tiny(r, kind)
        r.clear(CLEAR, 0.0)
        r.draw(r.upload_mesh(_tris7(sc, s), fr.VS_CLIP_COLOR), fr.PS_COLOR)
        r.sync()
        assert (r.stats()["replays"] >= 1) == want, f"{kind}: scene {s} alone, replays {r.stats()['replays']}"
        r.close()
    _CHECKED.add(kind)


class _Ctx:
    """A ctx on torch stream `st` in one of MODES, and the two ways its frames are read: a fenced copy on `st`, frr_readback"""

    def __init__(self, mode, kind=None):
        import torch
        import f_renderer_amd as fr
        self.torch, self.mode = torch, mode
        self.st = torch.cuda.Stream()
        self.r = fr.Renderer(W, H, stream=self.st.cuda_stream)
        if kind:
            _tiny(self.r, kind)
        self.sets, self.frame_no = None, 0
        if mode == "bound_in_flight":
            self.r.set_option("bound_targets_in_flight", 1)
            self.sets = [tuple(torch.zeros((H, W), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32))
                         for _ in range(3)]
        else:
            self.r.set_option("frames_in_flight", 1 if mode == "own_fif1" else 2)

    def frame(self, mesh, ps):
        r = self.r
        if self.sets:
            r.frame_wait(self.st.cuda_stream)     # the copies that still read this set (three frames back) come first
            r.bind_targets(*(x.data_ptr() for x in self.sets[self.frame_no % 3]))
        self.frame_no += 1
        r.clear(CLEAR, 0.0)
        r.draw(mesh, ps)

    def fenced_copy(self):
        """the current frame, copied on `st` behind frr_frame_fence -- no host wait, no frr_sync / frr_readback"""
        torch, st = self.torch, self.st
        self.r.frame_fence(st.cuda_stream)
        if self.sets:
            with torch.cuda.stream(st):
                return tuple(x.clone() for x in self.sets[(self.frame_no - 1) % 3])
        pc, pd, pt = self.r.target_ptrs()
        with torch.cuda.stream(st):
            return tuple(torch.as_tensor(_Alias(p, (H, W), ts), device="cuda").clone()
                         for p, ts in ((pc, "<i4"), (pd, "<f4"), (pt, "<i4")))

    def rewrite(self, buf, data):
        with self.torch.cuda.stream(self.st):
            buf.copy_(data)

    def close(self):
        self.torch.cuda.synchronize()
        self.r.close()


def _same_frame(f, c, d, t, what):
    """(c, d, t): torch tensors of a fenced copy or frr_readback's arrays, against oracle frame f"""
    as_np = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else x  # noqa: E731
    c, d, t = as_np(c), as_np(d), as_np(t)
    np.testing.assert_array_equal(t.view(np.uint32).ravel(), f.tri_id, err_msg=f"{what}: tri ids")
    np.testing.assert_array_equal(c.view(np.uint8).reshape(H, W, 4), f.color, err_msg=f"{what}: colour")
    assert_depth_equal(d.view(np.float32), f.depth, err_msg=f"{what}: depth")


@pytest.fixture(scope="module")
def select_shaders():
    """(slot-0 select, current-slot select) user shader ids (the registry is per process: compiled once)"""
    import f_renderer_amd as fr
    r = fr.Renderer(64, 64)
    ids = (r.register_shader(SELECT_SLOT0, 11, 3), r.register_shader(SELECT_CURRENT, 11, 3))
    r.close()
    return ids


def _rewrite_sequence(oracle, kind, mode, route):
    import torch
    import f_renderer_amd as fr
    _assert_not_vacuous(oracle, kind)
    sc = _scenes(oracle, kind)
    frames = sc[2]
    src = {s: torch.from_numpy(_tris7(sc, s)).to("cuda") for s in "LH"}
    buf = src["L"].clone()
    torch.cuda.synchronize()
    x = _Ctx(mode, kind)
    r = x.r
    m = r.bind_mesh_device(buf.data_ptr(), N_TRIS, fr.VS_CLIP_COLOR, keepalive=buf)
    copies = []
    for _ in range(2):                             # L: verified, and proven from now on (both workspace sets: passes alternate)
        x.frame(m, fr.PS_COLOR)
        copies.append(("L", x.fenced_copy()))
        _same_frame(frames["L"], *r.readback(), "readback of L")
    if route == "sync":                            # include/frr.h, frr_create: "frr_sync in place of (1) and (2)"
        r.sync()
        x.rewrite(buf, src["H"])
        r.sync()
    else:                                          # (1) fence the rewriting stream, (2) bind the mesh again
        r.frame_fence(x.st.cuda_stream)
        x.rewrite(buf, src["H"])
        m = r.bind_mesh_device(buf.data_ptr(), N_TRIS, fr.VS_CLIP_COLOR, keepalive=buf)
    x.frame(m, fr.PS_COLOR)                        # the same buffer, H in it now
    copies.append(("H", x.fenced_copy()))
    torch.cuda.synchronize()
    for s, cp in copies:
        _same_frame(frames[s], *cp, f"fenced copy of {s}")
    _same_frame(frames["H"], *r.readback(), "readback of H")
    x.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["bin", "fan"])
def test_in_place_rewrite_behind_sync_is_verified(oracle, kind, mode):
    """A device-bound mesh holding L is drawn (and proven); frr_sync, H written into the same buffer on the ctx's stream,
    frr_sync, the SAME mesh id drawn again: the pass must be verified (and replayed) before frr_draw returns."""
    _rewrite_sequence(oracle, kind, mode, "sync")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["bin", "fan"])
def test_in_place_rewrite_behind_fence_and_rebind(oracle, kind, mode):
    """Control: the same sequence by the fence-and-rebind route (a new registration: never proven)."""
    _rewrite_sequence(oracle, kind, mode, "rebind")


def _select_sequence(oracle, sid, switch):
    """A user-VS mesh whose positions follow a texel: drawn reading 0 (L), then `switch` makes it read 255 (H)"""
    import torch
    import f_renderer_amd as fr
    _assert_not_vacuous(oracle, "bin")
    sc = _scenes(oracle, "bin")
    x = _Ctx("own_fif2", "bin")
    r = x.r
    r.set_texture(0, _tex(0))
    r.set_texture(1, _tex(255))
    r.set_uniforms(texture_slot=0)
    m = r.upload_mesh(_tris11(sc, "L", "H"), sid)
    copies = []
    for _ in range(2):                             # (both workspace sets)
        x.frame(m, sid)
        copies.append(("L", x.fenced_copy()))
        _same_frame(sc[2]["L"], *r.readback(), "readback of L")
    switch(r)
    x.frame(m, sid)
    copies.append(("H", x.fenced_copy()))
    torch.cuda.synchronize()
    for s, cp in copies:
        _same_frame(sc[2][s], *cp, f"fenced copy of {s}")
    _same_frame(sc[2]["H"], *r.readback(), "readback of H")
    x.close()


def test_texture_reupload_under_a_sampling_user_vs(oracle, select_shaders):
    """frr::sample_2d_slot(u, 0, ...) in the vertex shader; slot 0 re-uploaded (0 -> 255) between two draws of one mesh"""
    _select_sequence(oracle, select_shaders[0], lambda r: r.set_texture(0, _tex(255)))


def test_texture_slot_switch_under_a_sampling_user_vs(oracle, select_shaders):
    """frr::sample_2d(u, ...) in the vertex shader; only uniforms.texture_slot changes (slot 0 holds 0, slot 1 255)"""
    _select_sequence(oracle, select_shaders[1], lambda r: r.set_uniforms(texture_slot=1))


def _beside(a, b):
    """do streams a and b run beside each other?  (a process's streams share a few hardware queues; two streams on one
    queue are ordered anyway, and a missing wait between them would go unseen)"""
    import torch
    ea, eb = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(a):
        torch.cuda._sleep(20_000_000)
        ea.record(a)
    eb.record(b)
    eb.synchronize()
    ok = not ea.query()
    ea.synchronize()
    return ok


def _streams_beside(k):
    """k torch streams that run pairwise beside each other"""
    import torch
    picked = []
    for _ in range(32):
        s = torch.cuda.Stream()
        if all(_beside(s, p) and _beside(p, s) for p in picked):
            picked.append(s)
        if len(picked) == k:
            return picked
    pytest.fail(f"no {k} streams on separate hardware queues")


def test_frame_wait_from_two_streams(oracle):
    """Two streams still read target set X (slowly); frr_frame_wait on each, then X is bound again and drawn into: the
    new frame must wait for BOTH readers."""
    import torch
    import f_renderer_amd as fr
    sc = _scenes(oracle, "bin")
    stA, stB, stC = _streams_beside(3)
    r = fr.Renderer(W, H, stream=stC.cuda_stream)
    r.set_option("overlap", 0)                     # (every kernel on stC: its queue is known to run beside A's and B's)
    X = tuple(torch.zeros((H, W), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32))
    ms = {s: r.upload_mesh(_tris7(sc, s), fr.VS_CLIP_COLOR) for s in "LH"}
    r.bind_targets(*(t.data_ptr() for t in X))
    r.clear(CLEAR, 0.0)
    r.draw(ms["H"], fr.PS_COLOR)
    r.sync()
    copies = []
    for st, cycles in ((stA, 60_000_000), (stB, 5_000_000)):   # (A is the slower reader: a lost edge to A shows)
        with torch.cuda.stream(st):
            torch.cuda._sleep(cycles)
            copies.append(tuple(t.clone() for t in X))
    r.frame_wait(stA.cuda_stream)
    r.frame_wait(stB.cuda_stream)
    r.bind_targets(*(t.data_ptr() for t in X))
    r.clear(CLEAR, 0.0)
    r.draw(ms["L"], fr.PS_COLOR)
    _same_frame(sc[2]["L"], *r.readback(), "readback of the new frame")
    torch.cuda.synchronize()
    for name, cp in zip("AB", copies):
        _same_frame(sc[2]["H"], *cp, f"stream {name}'s copy of the old frame")
    r.close()


def test_frame_wait_survives_a_pending_clear_of_another_binding(oracle):
    """Set X cleared without a draw (the clear is deferred), frr_frame_wait(st) while st still reads set Y, then Y bound,
    cleared and drawn into: X's clear (run by the bind) must not use up the wait -- Y's new frame waits for st."""
    import torch
    import f_renderer_amd as fr
    sc = _scenes(oracle, "bin")
    st, stC = _streams_beside(2)
    r = fr.Renderer(W, H, stream=stC.cuda_stream)
    r.set_option("overlap", 0)
    X, Y = (tuple(torch.zeros((H, W), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32))
            for _ in range(2))
    ms = {s: r.upload_mesh(_tris7(sc, s), fr.VS_CLIP_COLOR) for s in "LH"}
    r.bind_targets(*(t.data_ptr() for t in Y))
    r.clear(CLEAR, 0.0)
    r.draw(ms["H"], fr.PS_COLOR)
    r.sync()
    r.bind_targets(*(t.data_ptr() for t in X))
    r.clear(CLEAR, 0.0)                            # no draw: pending
    with torch.cuda.stream(st):
        torch.cuda._sleep(60_000_000)
        copy = tuple(t.clone() for t in Y)
    r.frame_wait(st.cuda_stream)
    r.bind_targets(*(t.data_ptr() for t in Y))     # settles X's clear
    r.clear(CLEAR, 0.0)
    r.draw(ms["L"], fr.PS_COLOR)
    _same_frame(sc[2]["L"], *r.readback(), "readback of Y's new frame")
    torch.cuda.synchronize()
    _same_frame(sc[2]["H"], *copy, "st's copy of Y's old frame")
    cleared = oracle.Frame(W, H)
    cleared.clear(CLEAR, 0.0)
    _same_frame(cleared, *X, "X after its clear")
    r.close()


# ---- model-based sequences ----------------------------------------------------------------------------------------------

STEPS = ("rewrite_sync", "rewrite_rebind", "texture", "slot", "user_uniforms", "draw", "fenced_read", "readback", "sync")


def _run_model(oracle, seed, sid):
    import torch
    import f_renderer_amd as fr
    sc = _scenes(oracle, "bin")
    frames = sc[2]
    rng = np.random.RandomState(seed)
    mode, overlap = MODES[seed % 3], (2, 0)[seed // 3 % 2]
    x = _Ctx(mode, "bin")
    r = x.r
    r.set_option("overlap", overlap)   # (0 with one frame in flight: every pass in one workspace set, proven by one draw)
    # the model: contents of the two device buffers, textures, texture_slot, u.user[0], the scene of the current frame
    model = {"c7": "L", "c11": ("L", "L"), "tex": [0, 0], "slot": 0, "user": 0.0, "frame": None}
    buf7 = torch.from_numpy(_tris7(sc, "L")).to("cuda")
    buf11 = torch.from_numpy(_tris11(sc, "L", "L")).to("cuda")
    torch.cuda.synchronize()
    ids = {7: r.bind_mesh_device(buf7.data_ptr(), N_TRIS, fr.VS_CLIP_COLOR, keepalive=buf7),
           11: r.bind_mesh_device(buf11.data_ptr(), N_TRIS, sid, keepalive=buf11)}
    for k in (0, 1):
        r.set_texture(k, _tex(0))
    r.set_uniforms(texture_slot=0)
    log, copies = [f"mode={mode} overlap={overlap}"], []
    p = np.array([2, 2, 1.5, 1.5, 1, 4, 3, 1, 1], np.float64)
    try:
        for _ in range(10):
            step = STEPS[rng.choice(len(STEPS), p=p / p.sum())]
            if step in ("rewrite_sync", "rewrite_rebind"):
                which = int(rng.choice([7, 11]))
                if which == 7:
                    new = "LH"[rng.randint(2)]
                    data = torch.from_numpy(_tris7(sc, new)).to("cuda")
                else:
                    new = ("LH"[rng.randint(2)], "LH"[rng.randint(2)])
                    data = torch.from_numpy(_tris11(sc, *new)).to("cuda")
                buf = buf7 if which == 7 else buf11
                log.append(f"{step}({which}={new})")
                x.st.wait_stream(torch.cuda.current_stream())   # (the upload of `data` above)
                if step == "rewrite_sync":
                    r.sync()
                    x.rewrite(buf, data)
                    r.sync()
                else:
                    r.frame_fence(x.st.cuda_stream)
                    x.rewrite(buf, data)
                    ids[which] = r.bind_mesh_device(buf.data_ptr(), N_TRIS, fr.VS_CLIP_COLOR if which == 7 else sid, keepalive=buf)
                data.record_stream(x.st)
                model["c7" if which == 7 else "c11"] = new
            elif step == "texture":
                k, v = rng.randint(2), int(rng.choice([0, 255]))
                log.append(f"texture({k}={v})")
                r.set_texture(k, _tex(v))
                model["tex"][k] = v
            elif step == "slot":
                model["slot"] ^= 1
                log.append(f"slot({model['slot']})")
                r.set_uniforms(texture_slot=model["slot"])
            elif step == "user_uniforms":
                model["user"] = float(rng.randint(2))
                log.append(f"user({model['user']})")
                r.set_user_uniforms([model["user"]])
            elif step == "draw":
                if rng.randint(2):
                    log.append("draw(builtin)")
                    x.frame(ids[7], fr.PS_COLOR)
                    model["frame"] = model["c7"]
                else:
                    hi = (model["tex"][model["slot"]] == 255) != (model["user"] > 0.5)
                    log.append("draw(user)")
                    x.frame(ids[11], sid)
                    model["frame"] = model["c11"][1 if hi else 0]
            elif model["frame"] is None:
                log.append(f"{step}(no frame yet)")
                if step == "sync":
                    r.sync()
            elif step == "fenced_read":
                log.append(f"fenced_read({model['frame']})")
                copies.append((len(log), model["frame"], x.fenced_copy()))
            elif step == "readback":
                log.append(f"readback({model['frame']})")
                _same_frame(frames[model["frame"]], *r.readback(), f"step {len(log)}: readback")
            else:
                log.append("sync")
                r.sync()
        torch.cuda.synchronize()
        for at, s, cp in copies:
            _same_frame(frames[s], *cp, f"step {at}: fenced copy")
    except AssertionError as e:
        raise AssertionError(f"seed {seed}, steps {log}:\n{e}") from None
    finally:
        x.close()


@pytest.mark.parametrize("seed", range(24))
def test_model_sequences(oracle, select_shaders, seed):
    """Random API sequences on tiny lists (rewrites of both device-bound meshes by both routes, texture uploads, slot
    switches, user uniforms, draws with the built-in or the texel-select VS, fenced reads, readbacks, syncs), every frame
    read held to the model's scene."""
    _assert_not_vacuous(oracle, "bin")
    _run_model(oracle, seed, select_shaders[1])
