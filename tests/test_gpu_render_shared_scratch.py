"""Every render entry point fills the scratch it is given itself: the five renderers share one z-buffer kernel, one
rasteriser and one host preamble, and their keys differ in form (millimetres, or millimetres << 16 | label), so a call
must not see what the call before it left.  All six calls back to back on one stream through one scratch, each compared
byte for byte with the same call on a scratch of its own."""
import ctypes

import numpy as np
import pytest
import torch

import label_render_ref as lr
import render_depth_ref as rd
import test_gpu_splat_depth as tg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, STRIDE, NF, ZN = 50, 70, 2, 3, 0.25


def test_back_to_back_calls_share_one_scratch():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    _, inv, soa, lab = lr.label_cloud(70)
    dh, dw = rd.rendered_size(H, W, STRIDE)
    xyz = torch.from_numpy(soa).to(DEV)
    poses = torch.from_numpy(inv[:NF].copy()).to(DEV)
    labels = torch.from_numpy(lab[:tg.N].view(np.int16).copy()).to(DEV)
    rng = np.random.default_rng(3)                                       # a mesh over the cloud: near neighbours along x and
    faces = np.concatenate([np.sort(rng.integers(0, 40, (150, 3)), 1) + rng.integers(24, tg.N - 40, (150, 1)),
                            rng.integers(0, tg.N, (50, 3))]).astype(np.int32)    # triangles across the scene (and the crafted points)
    faces = torch.from_numpy(faces).to(DEV)
    k9 = ctypes.cast((ctypes.c_double * 9)(*tg.K33.reshape(-1).tolist()), ctypes.c_void_p)
    P = _lib._ptr
    cloud = (P(xyz), tg.N, tg.N_PAD)
    mesh = cloud + (P(faces), int(faces.shape[0]))
    view = (P(poses), k9, NF, H, W, dh, dw)

    def six_calls(scratch):
        """The six calls in order, back to back on the current stream with no synchronise in between, each through
        scratch() -> their seven frames (the first labelled call also writes its depth, the second leaves it out)."""
        o = [torch.full((NF, dh, dw), 7, dtype=torch.int16, device=DEV) for _ in range(7)]
        _lib.call("bff_render_labels_u16", *cloud, P(labels), *view, tg.R, 0, scratch(), P(o[0]), P(o[1]), None)
        _lib.call("bff_render_depth_u16", *cloud, *view, 0, scratch(), P(o[2]), None)
        _lib.call("bff_render_splat_depth_u16", *cloud, *view, tg.R, 0, scratch(), P(o[3]), None)
        _lib.call("bff_render_mesh_depth_u16", *mesh, *view, 0, scratch(), P(o[4]))
        _lib.call("bff_render_mesh_depth_clip_u16", *mesh, *view, ZN, 0, scratch(), P(o[5]))
        _lib.call("bff_render_labels_u16", *cloud, P(labels), *view, 0.0, 0, scratch(), P(o[6]), None, None)
        torch.cuda.synchronize()
        return o

    shared = torch.zeros(NF * dh * dw, dtype=torch.int32, device=DEV)    # zeros: a key that would win every minimum
    got = six_calls(lambda: P(shared))
    fresh = []                                                           # one scratch per call, alive until the calls have run
    alone = six_calls(lambda: (fresh.append(torch.full_like(shared, 7)), P(fresh[-1]))[1])
    assert len(fresh) == 6
    for name, a, b in zip(("labels", "labels' depth", "points", "splat", "mesh", "clipped mesh", "labels at radius 0"), got, alone):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), name
    assert all(int(t.count_nonzero()) for t in alone)                    # every call drew something
    assert not torch.equal(alone[2], alone[3]) and not torch.equal(alone[0], alone[6])   # the calls differ from one another
