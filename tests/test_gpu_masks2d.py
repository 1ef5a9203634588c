"""Dense 2-D masks -> run tables / RLE on the device (bff_masks2d_count + bff_masks2d_runs, masks2d.py) against the
oracle's rle_encode_batch, the shipped decoder and the reference-generated fixtures; and the hand-off: a scene whose
mask_2d entries are dense tensors or DeviceRuns gives the same DeviceScene and the same stage-2 result as its RLE twin
through the general, fast, multi-class and Ingestor paths."""
import os
import warnings

import numpy as np
import pytest
import torch

import golden_io as gio
from oracle import rle_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Z = lambda name: np.load(os.path.join(gio.GOLDEN_DIR, name))


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def edge_rows(n, seed):
    """The row set of test_rows_to_rle_matches_reference_encoder: empty, full, p < 0.5, sparse with first and last pixel
    set, dense with holes, blocks of 37, even pixels, odd pixels."""
    rng = np.random.default_rng(seed)
    d = np.stack([rng.random(n) < p for p in (0.0, 1.0, 0.5, 0.02, 0.98)] +
                 [np.repeat(rng.random(n // 37 + 1) < 0.5, 37)[:n], np.arange(n) % 2 == 0, np.arange(n) % 2 == 1])
    d[3, 0] = d[3, -1] = True
    return d


def same_rles(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g["length"] == e["length"]
        assert g["counts"].dtype == e["counts"].dtype == np.int64 and np.array_equal(g["counts"], e["counts"])


def check_against_oracle(lib, dense_dev, dense_np):
    """dense_dev: what is handed to encode_masks; dense_np: bool (M, P), what it means.  Everything item 1 of the kernel
    parity asks for: RLE dicts, int32 tables, the round trip through the shipped decoder, the bit planes."""
    from beyond_fixed_forms_amd import masks2d
    from beyond_fixed_forms_amd.scene import runs_from_rles
    m, n = dense_np.shape
    runs = masks2d.encode_masks(dense_dev)
    assert len(runs) == m == runs.n_masks and runs.n_pixels == n
    exp = rle_ref.rle_encode_batch_ref(torch.from_numpy(dense_np))
    same_rles(runs.to_rles(), exp)
    for got, e in zip((runs.run_start, runs.run_end, runs.mask_run_offs), runs_from_rles(exp)):
        assert got.dtype == torch.int32 and got.is_cuda and torch.equal(got.cpu(), torch.from_numpy(e))
    # the shipped decoder: all masks as mask-views of <= 32 masks, 32-bit words
    vmo = torch.tensor(list(range(0, m, 32)) + [m], dtype=torch.int32, device=DEV)
    maskbits = torch.empty((vmo.shape[0] - 1, n), dtype=torch.int32, device=DEV)
    lib.rle_to_maskbits(runs.run_start, runs.run_end, runs.mask_run_offs, vmo, vmo.shape[0] - 1, n, 32, maskbits)
    mb = maskbits.cpu().numpy().view(np.uint32)
    back = np.stack([(mb[g // 32] >> np.uint32(g % 32)) & 1 for g in range(m)]).astype(bool)
    assert np.array_equal(back, dense_np)
    # the count pass on its own: bit planes in bff_pack_rows' layout, counts = the tables' row sizes
    rows8 = torch.from_numpy(dense_np).to(DEV).view(torch.uint8)
    bits = torch.full((m, (n + 63) // 64), -1, dtype=torch.int64, device=DEV)
    counts = torch.full((m,), 12345, dtype=torch.int32, device=DEV)          # written, not accumulated
    lib.masks2d_count(rows8, bits, counts)
    assert torch.equal(bits, lib.pack_rows(rows8))
    assert torch.equal(counts, runs.mask_run_offs[1:] - runs.mask_run_offs[:-1])
    return runs


def parity_sizes():
    from beyond_fixed_forms_amd.masks2d import TILE_PIXELS as T
    return [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T + 1, 120 * 160, 121 * 163]


@pytest.mark.parametrize("n", parity_sizes())
def test_encoder_matches_reference_encoder(lib, n):
    """Item 1: sizes around every internal boundary (16-pixel lane loads, 64-pixel words, 1024-pixel wave stretches,
    the block tile), odd sizes that misalign every mask but the first."""
    from beyond_fixed_forms_amd.masks2d import TILE_PIXELS
    assert lib.load().bff_masks2d_tile_pixels() == TILE_PIXELS
    d = edge_rows(n, n)
    check_against_oracle(lib, torch.from_numpy(d).to(DEV), d)


def test_nonzero_means_set_and_strided_input(lib):
    """Item 2: any non-zero byte is a set pixel; a (M,1,H,W) bool view that is not contiguous; a host tensor; (M,H,W)."""
    from beyond_fixed_forms_amd import masks2d
    rng = np.random.default_rng(5)
    h, w, m = 37, 53, 5
    vals = np.array([0, 1, 2, 128, 255], dtype=np.uint8)[rng.integers(0, 5, (m, h * w))]
    vals[:, :40] = np.array([0, 0, 2, 128, 0, 255, 1, 0] * 5, dtype=np.uint8)
    check_against_oracle(lib, torch.from_numpy(vals).to(DEV), vals != 0)
    big = torch.from_numpy(rng.random((m, 1, h + 3, w + 5)) < 0.5).to(DEV)
    view = big[:, :, 1:h + 1, 2:w + 2]
    assert not view.is_contiguous() and view.dtype == torch.bool
    flat = view.cpu().numpy().reshape(m, -1)
    a = check_against_oracle(lib, view, flat)
    for form in (view.cpu(), view[:, 0], view.contiguous().view(m, -1)):         # host tensor, (M,H,W), (M,H*W)
        b = masks2d.encode_masks(form)
        assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("run_start", "run_end", "mask_run_offs"))
    with pytest.raises(TypeError):
        masks2d.encode_masks(view.float())
    with pytest.raises(ValueError):
        masks2d.encode_masks(torch.zeros((2, 3, 4, 5), dtype=torch.bool, device=DEV))


def test_runs_across_every_internal_boundary(lib):
    """Item 3: runs that start and end exactly at, one before and one after each multiple of 16, 64, 1024 and the tile
    size (multiples of 16 cover them all), long runs across the 1024-pixel stretches and the tiles, one single run
    covering everything."""
    from beyond_fixed_forms_amd.masks2d import TILE_PIXELS as T
    n = 3 * T + 77
    rows = []
    for d in (-1, 0, 1):
        starts_at = np.zeros(n, dtype=bool)              # a run of 5 starting at every 16 k + d
        ends_at = np.zeros(n, dtype=bool)                # a run of 5 ending (exclusive) at every 16 k + d
        for b in range(0, n + 16, 16):
            lo, hi = max(b + d, 0), min(b + d + 5, n)
            if lo < hi:
                starts_at[lo:hi] = True
            lo, hi = max(b + d - 5, 0), min(b + d, n)
            if lo < hi:
                ends_at[lo:hi] = True
        across = np.zeros(n, dtype=bool)                 # runs from 1024 k + d + 2 to 1024 (k + 1) + d
        for b in range(0, n, 1024):
            across[max(b + d + 2, 0):min(b + 1024 + d, n)] = True
        rows += [starts_at, ends_at, across]
    tiles = np.ones(n, dtype=bool)                       # runs that end one before / begin one after every tile boundary
    tiles[T - 1::T] = False
    rows += [tiles, np.ones(n, dtype=bool)]
    d = np.stack(rows)
    check_against_oracle(lib, torch.from_numpy(d).to(DEV), d)


def test_masks_at_the_end_of_their_allocation(lib):
    """Item 3: the last mask's last byte is the last byte of the allocation (an odd H*W: the last 16-pixel piece is
    partial and every mask base misaligned); the result equals that of a copy placed elsewhere."""
    from beyond_fixed_forms_amd import masks2d
    m, p = 3, 121 * 163
    d = edge_rows(p, 9)[[2, 1, 3]]                       # the last mask has its last pixel set, the middle one is full
    total = 20 << 20
    buf = torch.empty(total, dtype=torch.uint8, device=DEV)
    at_end = buf.narrow(0, total - m * p, m * p).view(m, p)
    at_end.copy_(torch.from_numpy(d).to(DEV))
    assert at_end.data_ptr() + m * p == buf.data_ptr() + total
    other = torch.empty(m * p + 64, dtype=torch.uint8, device=DEV)[3:3 + m * p].view(m, p)
    other.copy_(at_end)
    a, b = masks2d.encode_masks(at_end), masks2d.encode_masks(other)
    for k in ("run_start", "run_end", "mask_run_offs"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    same_rles(a.to_rles(), rle_ref.rle_encode_batch_ref(torch.from_numpy(d)))


def count_fetches(monkeypatch):
    from beyond_fixed_forms_amd import masks2d
    calls, real = [], masks2d._fetch_runs

    def counting(*tensors):
        calls.append(len(tensors))
        return real(*tensors)
    monkeypatch.setattr(masks2d, "_fetch_runs", counting)
    return calls


def test_reference_generated_fixtures(lib, monkeypatch):
    """Item 4: what the reference's own encode_2d_masks / rle_encode_batch wrote (tests/golden/refine_helpers.npz) comes
    out of masks2d.encode_2d_masks bit for bit; list forms; one device-to-host copy of runs per call."""
    from beyond_fixed_forms_amd import masks2d
    z = Z("refine_helpers.npz")
    m2 = torch.from_numpy(z["rle2d.dense"])
    exp2 = gio.unpack_rles(z["rle2d.len"], z["rle2d.counts"], z["rle2d.offs"])
    batch = torch.from_numpy(z["rlebatch.dense"])
    expb = gio.unpack_rles(z["rlebatch.len"], z["rlebatch.counts"], z["rlebatch.offs"])
    assert m2.dim() == 4 and m2.dtype == torch.bool and batch.dim() == 2
    calls = count_fetches(monkeypatch)
    frames = masks2d.encode_2d_masks([{"segmented_frame_masks": m2.clone().to(DEV)}])
    assert calls == [3]                                               # start, end, offsets: one synchronisation
    same_rles(frames[0]["segmented_frame_masks"], exp2)
    del calls[:]
    same_rles(masks2d.encode_masks(batch.to(DEV)).to_rles(), expb)
    assert len(calls) == 1
    # several frames in one call, one without masks, one already in RLE form (left alone), one on the host
    h, w = m2.shape[2:]
    already = [dict(length=h * w, counts=np.array([2, 3], dtype=np.int64))]
    empty = torch.zeros((0, 1, h, w), dtype=torch.bool, device=DEV)
    flipped = ~m2
    lst = [{"segmented_frame_masks": m2.to(DEV), "frame_id": "0.jpg"}, {"segmented_frame_masks": empty},
           {"segmented_frame_masks": already}, {"segmented_frame_masks": flipped}, {"segmented_frame_masks": m2[:1].to(DEV)}]
    del calls[:]
    out = masks2d.encode_2d_masks(lst)
    assert len(calls) == 1 and out is lst and lst[0]["frame_id"] == "0.jpg"
    same_rles(lst[0]["segmented_frame_masks"], exp2)
    assert lst[1]["segmented_frame_masks"] == [] and lst[2]["segmented_frame_masks"] is already
    same_rles(lst[3]["segmented_frame_masks"], rle_ref.rle_encode_batch_ref(flipped.view(flipped.shape[0], -1)))
    same_rles(lst[4]["segmented_frame_masks"], exp2[:1])
    # encode_masks on a list: one DeviceRuns per frame, views into shared tables, nothing fetched
    del calls[:]
    per = masks2d.encode_masks([m2.to(DEV), empty, flipped.to(DEV)])
    assert calls == [] and [len(p) for p in per] == [m2.shape[0], 0, m2.shape[0]]
    assert per[0].run_start.data_ptr() == per[2].run_start.data_ptr()
    same_rles(per[0].to_rles(), exp2)
    same_rles(per[2].to_rles(), rle_ref.rle_encode_batch_ref(flipped.view(flipped.shape[0], -1)))
    assert per[1].to_rles() == []
    # nothing at all
    assert masks2d.encode_masks([]) == [] and masks2d.encode_2d_masks([]) == []
    assert len(masks2d.encode_masks(empty)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# hand-off

def cfg_for(scene, **over):
    from beyond_fixed_forms_amd.config import Config
    return Config.with_defaults(width_2d=scene.width, height_2d=scene.height, **over)


def densify(scene, mask_2d, which=lambda i: True):
    """The dense twin of a mask_2d list: entry i decoded by the oracle into a bool (M,1,H,W) device tensor (if which(i))."""
    out = []
    for i, fr in enumerate(mask_2d):
        rl = fr["segmented_frame_masks"]
        if which(i):
            d = rle_ref.rle_decode_batch_ref(rl).view(len(rl), 1, scene.height, scene.width).bool().to(DEV) if len(rl) \
                else torch.zeros((0, 1, scene.height, scene.width), dtype=torch.bool, device=DEV)
            fr = dict(fr, segmented_frame_masks=d)
        out.append(fr)
    return out


TABLES = ("run_start", "run_end", "mask_run_offs", "view_mask_offs", "depth_index", "frame_mask", "frame_rowbase",
          "frame_nmask", "frame_flags", "conf", "label_id", "inv_pose")


def same_device_scene(a, b):
    for k in TABLES:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and torch.equal(x, y), k
    assert (a.n_frames, a.n_mask_frames, a.n_viewed, a.word_bits, a.n_rows, a.labels) == \
           (b.n_frames, b.n_mask_frames, b.n_viewed, b.word_bits, b.n_rows, b.labels)


def same_result(got, exp):
    if isinstance(exp["ins"], list):
        assert got["ins"] == [] and got["conf"] == [] and got["final_class"] == []
        return
    assert got["ins"].dtype == exp["ins"].dtype and torch.equal(got["ins"].cpu(), exp["ins"].cpu())
    assert got["conf"].dtype == exp["conf"].dtype and torch.equal(got["conf"].cpu(), exp["conf"].cpu())
    assert list(got["final_class"]) == list(exp["final_class"])


def forms_of(scene):
    """The scene with its masks dense, as DeviceRuns, and mixed (even entries dense, odd ones RLE)."""
    from beyond_fixed_forms_amd import masks2d
    from beyond_fixed_forms_amd.synthetic import class_scene
    dense = densify(scene, scene.mask_2d)
    return {"dense": class_scene(scene, dense), "device_runs": class_scene(scene, masks2d.to_device_runs(dense)),
            "mixed": class_scene(scene, densify(scene, scene.mask_2d, lambda i: i % 2 == 0))}


def check_all_paths(scene, cfg):
    from beyond_fixed_forms_amd.ingest import prepare_scene_fast
    from beyond_fixed_forms_amd.projection import project_scene
    from beyond_fixed_forms_amd.scene import prepare_scene
    ref_ds = prepare_scene(scene, cfg, device=DEV)
    ref = project_scene(scene, cfg, DEV)
    for name, twin in forms_of(scene).items():
        same_device_scene(prepare_scene(twin, cfg, device=DEV), ref_ds)
        same_device_scene(prepare_scene_fast(twin, cfg, device=DEV), ref_ds)
        same_result(project_scene(twin, cfg, DEV), ref)
    return ref


@pytest.mark.parametrize("mode", ["ratio", "occurrence"])
@pytest.mark.parametrize("seed", [0, 1])
def test_handoff_tiny_scene(lib, seed, mode):
    """Item 5: prepare_scene / prepare_scene_fast / project_scene on the dense twin, its to_device_runs form and a mixed
    list == on the RLE original, and the original == the oracle."""
    from beyond_fixed_forms_amd.synthetic import make_scene
    from oracle.projection_ref import project_scene_ref
    scene = make_scene("tiny", seed)
    cfg = cfg_for(scene, **({} if mode == "ratio" else dict(if_occurance_threshold=True)))
    got = check_all_paths(scene, cfg)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        same_result(got, project_scene_ref(scene, cfg))


@pytest.mark.parametrize("n_masks", [33, 70])
def test_handoff_many_masks_per_frame(lib, n_masks):
    """33 masks in a frame: 64-bit mask words; 70: the frame is split into two mask-views."""
    from beyond_fixed_forms_amd.scene import prepare_scene
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", 2, n_masks=n_masks)
    cfg = cfg_for(scene)
    check_all_paths(scene, cfg)
    ds = prepare_scene(forms_of(scene)["dense"], cfg, device=DEV)
    assert ds.word_bits == 64 and ds.n_mask_frames == len(scene.mask_2d) * (1 if n_masks <= 64 else 2)


def test_handoff_empty_frame_and_subsets(lib):
    """An entry whose tensor holds no mask makes no kernel frame; a subset of the entries of one to_device_runs call
    (its runs are then gathered on the device) and DeviceRuns of separate encode_masks calls (concatenated)."""
    from beyond_fixed_forms_amd import masks2d
    from beyond_fixed_forms_amd.scene import prepare_scene
    from beyond_fixed_forms_amd.synthetic import class_scene, make_scene
    base = make_scene("tiny", 3)
    cfg = cfg_for(base)
    fr = base.mask_2d[1]
    hollow = list(base.mask_2d)
    hollow[1] = dict(fr, segmented_frame_masks=[], confidences=fr["confidences"][:0], labels=[])
    scene = class_scene(base, hollow)
    check_all_paths(scene, cfg)
    dense = densify(scene, scene.mask_2d)
    assert dense[1]["segmented_frame_masks"].shape[0] == 0
    assert prepare_scene(class_scene(scene, dense), cfg, device=DEV).n_mask_frames == len(hollow) - 1
    runs = masks2d.to_device_runs(densify(base, base.mask_2d))
    keep = [0, 2, 3]
    same_device_scene(prepare_scene(class_scene(base, [runs[i] for i in keep]), cfg, device=DEV),
                      prepare_scene(class_scene(base, [base.mask_2d[i] for i in keep]), cfg, device=DEV))
    apart = [dict(fr, segmented_frame_masks=masks2d.encode_masks(d["segmented_frame_masks"]))
             for fr, d in zip(base.mask_2d, densify(base, base.mask_2d))]
    same_device_scene(prepare_scene(class_scene(base, apart), cfg, device=DEV), prepare_scene(base, cfg, device=DEV))


def test_handoff_classes(lib):
    """project_scene_classes with two derived classes, one dense and one RLE == both RLE."""
    from beyond_fixed_forms_amd.projection import project_scene_classes
    from beyond_fixed_forms_amd.synthetic import derive_classes, make_scene
    for seed in (0, 1):
        scene = make_scene("tiny", seed)
        cfg = cfg_for(scene)
        masks = derive_classes(scene, k=2, fraction=0.5, seed=seed)
        a, b = list(masks)
        exp = project_scene_classes(scene, masks, cfg, DEV)
        for twin in ({a: densify(scene, masks[a]), b: masks[b]}, {a: masks[a], b: densify(scene, masks[b])}):
            for debug_out in (False, True):                           # prepare_class_fast / prepare_class
                got = project_scene_classes(scene, twin, cfg, DEV, debug_out=debug_out)
                for c in masks:
                    same_result(got[c], exp[c])


def test_handoff_ingestor(lib):
    """Ingestor.submit on dense / DeviceRuns scenes: loader threads encode on their own streams."""
    from beyond_fixed_forms_amd import ingest
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.synthetic import make_scene
    scenes = [make_scene("tiny", s) for s in (0, 1)]
    cfg = cfg_for(scenes[0])
    items = []
    for sc in scenes:
        f = forms_of(sc)
        items += [(sc, sc), (sc, f["dense"]), (sc, f["device_runs"])]
    torch.cuda.synchronize()                             # the twins' tensors are complete before loader streams read them
    ing = ingest.Ingestor(cfg, DEV, n_loaders=2, native_threads=2, with_stage1=False)
    try:
        futs = [ing.submit(twin) for _, twin in items]
        out = []
        for f in futs:
            ds, _, ev = f.result()
            ev.synchronize()
            out.append(ds)
    finally:
        ing.close()
    for k in range(0, len(items), 3):
        same_device_scene(out[k + 1], out[k])
        same_device_scene(out[k + 2], out[k])
        exp = run_projection(out[k], cfg).to_dict()
        same_result(run_projection(out[k + 1], cfg).to_dict(), exp)
        same_result(run_projection(out[k + 2], cfg).to_dict(), exp)


def test_handoff_refuses_wrong_sizes_and_dtypes(lib):
    from beyond_fixed_forms_amd import masks2d
    from beyond_fixed_forms_amd.ingest import prepare_scene_fast
    from beyond_fixed_forms_amd.scene import prepare_scene
    from beyond_fixed_forms_amd.synthetic import class_scene, make_scene
    scene = make_scene("tiny", 0)
    cfg = cfg_for(scene)
    dense = densify(scene, scene.mask_2d)
    h, w = scene.height, scene.width

    def with_first(t):
        return class_scene(scene, [dict(dense[0], segmented_frame_masks=t)] + dense[1:])
    m = dense[0]["segmented_frame_masks"].shape[0]
    taller = torch.zeros((m, 1, h + 1, w), dtype=torch.bool, device=DEV)
    for prep in (prepare_scene, prepare_scene_fast):
        with pytest.raises(ValueError, match=r"mask RLE length \d+ != H\*W"):
            prep(with_first(taller), cfg, device=DEV)
        with pytest.raises(ValueError, match=r"mask RLE length \d+ != H\*W"):
            prep(with_first(masks2d.encode_masks(taller)), cfg, device=DEV)
        with pytest.raises(TypeError):
            prep(with_first(dense[0]["segmented_frame_masks"].float()), cfg, device=DEV)
