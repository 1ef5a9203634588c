"""Command-line drop-ins with the reference's argv (`--config <yaml> --cls "<query>"`), file layout,
checkpoints and exit-code contract: exit code 0 on success, any exception
propagates to a non-zero exit, empty results are saved, not errors.

One process per GPU.  `BFF_GPUS=<n>|all` makes either script start n ranks of itself under
`python -m torch.distributed.run` (decided before anything touches the GPU; the child's exit code is
returned, so `run_evl.py`'s `subprocess.run(check=True)` sees one process as before); a script that finds RANK /
WORLD_SIZE in its environment (torchrun) IS a rank.  Scenes are dealt to the ranks by `distributed.shard_scenes`;
every rank reads, ingests (loader threads, `ingest.Ingestor`) and projects its shard with PIPELINE_DEPTH scenes in
flight (`pipeline.project_stream`).  The refinement makes the class's one exchange and one gather
(`distributed.ClassBatch`) and rank 0 writes the final files; the projection stage's files are the hand-over between
the two processes and are written by the rank that produced them (their `final_class` strings come from that rank's
mask_2d file), the class checkpoint by rank 0.

The third stage, `evaluation_main` (the reference's evaluation/eval/eval_scannet200.py), scores a class's final files
against the ground truth in one process: AP, AP50, AP25 and the recalls into the class's line of the results file.
Beside the path: `reproject_main` renders a stage's instances back into the colour frames as 2-D masks, `split_main` cuts
them into their spatially connected parts, `cluster_main` into their density clusters, `snap_main` snaps them to the
scan's superpoints, `subsample_main` writes a voxel subsample of every cloud and `lift_main` carries the instances of a run
on it back to the full cloud, and `assemble_main` gathers a scene's instances of all classes into one prediction, duplicates
removed by a 3-D mask NMS (`evaluation_main --assembled` scores it), and `select_views_main` finds the frames that see each
instance best and the boxes to crop it with; each writes to a directory of its own.  The four that turn a stage's files into files of
the same format (split, cluster, snap, lift) are one driver, `_stage_main`, with a per-scene function each.
"""
from __future__ import annotations

import argparse
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .config import load_config
from .io import (load_scene, read_scene_checkpoint, save_result, write_scene_checkpoint)
from .refinement import TextSimilarity


def _parser(desc):
    p = argparse.ArgumentParser(description=desc)                 # P:314-318 / R:128-132
    p.add_argument("--config", type=str, required=True, help="Config")
    p.add_argument("--cls", type=str, required=True, help="Class")
    return p


def _stage_parser(desc):
    p = _parser(desc)
    p.add_argument("--stage", type=str, default="final", choices=("final", "mask_3d"),
                   help="Whose instances: the refinement's (final_output_dir) or the projection stage's (mask_3d_dir)")
    return p


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(argv=None):
    """BFF_GPUS=<n>|all and not yet a rank: run n ranks of this very script under torch.distributed.run as a child
    process and return its exit code (None: stay a single process).  Nothing here initialises the GPU
    (`torch.cuda.device_count()` does not on this platform), so the launcher is chosen before any HIP call."""
    want = os.environ.get("BFF_GPUS", "").strip().lower()
    if not want or "RANK" in os.environ or "WORLD_SIZE" in os.environ:
        return None
    n = torch.cuda.device_count() if want == "all" else int(want)
    if n <= 1:
        return None
    args = list(sys.argv[1:] if argv is None else argv)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(sys.argv[0])] + args
    return subprocess.run(cmd).returncode


def _host_threads():
    """The host side makes only tiny torch CPU calls; by default each opens an OpenMP region as wide as the machine
    (times the ranks of a node).  BFF_TORCH_THREADS overrides (0: leave torch's setting alone)."""
    n = int(os.environ.get("BFF_TORCH_THREADS", "4"))
    if n > 0:
        torch.set_num_threads(n)


def init_ranks():
    """-> (rank, world size, device).  Under torchrun: one GPU per rank over RCCL (backend "nccl");
    BFF_REHEARSE_ON_ONE_GPU=1 puts every rank on cuda:0 with gloo collectives -- only to rehearse the N > 1 code
    path on a single-GPU box."""
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    if ws <= 1:
        return 0, 1, "cuda"
    rehearse = os.environ.get("BFF_REHEARSE_ON_ONE_GPU") == "1"
    local = 0 if rehearse else int(os.environ.get("LOCAL_RANK", "0"))
    if rehearse:
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
    torch.cuda.set_device(local)
    return dist.get_rank(), ws, f"cuda:{local}"


def _finish_ranks():
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def _coll_device(device):
    return device if dist.get_backend() == "nccl" else "cpu"


def _projection_parser():
    """P:314-318, with --cls repeatable: several query classes in one run (each scene read and uploaded once)."""
    p = argparse.ArgumentParser(description="Beyond-Fixed-Forms 2D->3D projection (MI355X)")
    p.add_argument("--config", type=str, required=True, help="Config")
    p.add_argument("--cls", type=str, required=True, action="append",
                   help="Class; give it more than once to project several classes in one run")
    return p


def projection_main(argv=None):
    """python tools/projection_2d_to_3d.py --config configs/config.yaml --cls "<class>" [--cls "<class>" ...]
    (P:336-634).  One --cls: the reference's run.  Several: every class's files, checkpoint and log lines exactly as
    its own run writes them, each scene read, uploaded and viewed-counted once for all of its classes."""
    args = _projection_parser().parse_args(argv)
    rc = launch_ranks(argv)
    if rc is not None:
        return rc
    cfg = load_config(args.config)
    _lib.load()
    _host_threads()
    classes = list(dict.fromkeys(args.cls))
    if len(classes) > 1:
        return _projection_classes(cfg, classes)
    cls = classes[0]
    from .distributed import shard_scenes
    from .pipeline import project_stream
    rank, ws, device = init_ranks()
    ckpt = read_scene_checkpoint("projection_2d_to_3d", cls)
    seg_dir = os.path.join(cfg.mask_2d_dir, cls)
    scene_ids = [s[:-4] for s in sorted(s for s in os.listdir(seg_dir) if s.endswith("_00.pth"))]   # P:363
    # heavier scenes first when dealing them to the ranks: the cloud file's size stands for N
    weights = None
    if ws > 1:
        weights = [os.path.getsize(p) if os.path.exists(p) else 0
                   for p in (os.path.join(cfg.scene_npy_dir, f"{s}.npy") for s in scene_ids)]
    mine = shard_scenes(scene_ids, rank, ws, weights)
    # BFF_DEPTH_ON_DEVICE=1: upload the 16-bit depth PNGs as they are, scale + resize them on the GPU
    on_dev = os.environ.get("BFF_DEPTH_ON_DEVICE") == "1"
    # the files of the next scenes (point cloud, ~300 depth PNGs, poses, the mask dict) are read and uploaded by loader
    # threads while the GPU works on the current ones; a load error surfaces at that scene's turn, after the earlier
    # scenes are saved
    sources = [functools.partial(load_scene, cfg, cls, scene_ids[i], depth_on_device=on_dev) for i in mine]
    done = []

    def consume(k, _st1, res):
        scene_id = scene_ids[mine[k]]
        print("Working on", scene_id, "class", cls)
        if not res.debug.get("empty_form", False):
            done.append(mine[k])
            if ws == 1:
                ckpt[scene_id] = True                                                     # P:580-581
                write_scene_checkpoint("projection_2d_to_3d", cls, ckpt)
        # BFF_SAVE_RLE=1 stores "ins" as RLE dicts (Open3DIS format; refinement.py and eval_scannet200.py:123-124
        # read both forms) instead of the reference's dense bool matrix
        out = res.to_rle_dict() if os.environ.get("BFF_SAVE_RLE") == "1" and not res.debug.get("empty_form") else res.to_dict()
        save_result(out, cfg.mask_3d_dir, cls, scene_id)                                    # P:630-634

    project_stream(sources, cfg, device, consume, n_loaders=int(os.environ.get("BFF_LOADERS", "2")), with_stage1=False)
    if ws > 1:
        # one small reduction tells rank 0 which scenes were completed anywhere; it alone writes the class checkpoint
        flags = torch.zeros(max(len(scene_ids), 1), dtype=torch.int32, device=_coll_device(device))
        if done:
            flags[torch.tensor(done, dtype=torch.long)] = 1
        dist.reduce(flags, dst=0, op=dist.ReduceOp.SUM)
        if rank == 0:
            for i in torch.nonzero(flags.cpu()).view(-1).tolist():
                ckpt[scene_ids[i]] = True
            write_scene_checkpoint("projection_2d_to_3d", cls, ckpt)
        _finish_ranks()
    return 0


def class_scenes(mask_2d_dir, classes):
    """Scenes of a multi-class run: each class's own listing mask_2d/<cls>/*_00.pth (P:363), their union in sorted
    order, and for every scene the classes that list it, in the given order.  -> (scene ids, [classes per scene])."""
    lists = {c: {s[:-4] for s in os.listdir(os.path.join(mask_2d_dir, c)) if s.endswith("_00.pth")} for c in classes}
    scene_ids = sorted(set().union(*lists.values()))
    return scene_ids, [[c for c in classes if sid in lists[c]] for sid in scene_ids]


def _projection_classes(cfg, classes):
    """The projection stage for several classes: scenes = the union of the classes' mask_2d listings (P:363) in sorted
    order, each projected for the classes that list it, in command-line order (pipeline.project_classes_stream)."""
    from .distributed import shard_scenes
    from .io import load_scene_classes
    from .pipeline import project_classes_stream
    rank, ws, device = init_ranks()
    ckpts = {c: read_scene_checkpoint("projection_2d_to_3d", c) for c in classes}
    scene_ids, per_scene = class_scenes(cfg.mask_2d_dir, classes)
    weights = None
    if ws > 1:
        weights = [os.path.getsize(p) if os.path.exists(p) else 0
                   for p in (os.path.join(cfg.scene_npy_dir, f"{s}.npy") for s in scene_ids)]
    mine = shard_scenes(scene_ids, rank, ws, weights)
    on_dev = os.environ.get("BFF_DEPTH_ON_DEVICE") == "1"
    items = []
    for i in mine:
        items.append((functools.partial(load_scene_classes, cfg, per_scene[i], scene_ids[i], depth_on_device=on_dev),
                       per_scene[i]))
    done = []                                   # (class index, scene index) of the non-empty results

    def consume(k, cls, _st1, res):
        scene_id = scene_ids[mine[k]]
        print("Working on", scene_id, "class", cls)
        if not res.debug.get("empty_form", False):
            done.append((classes.index(cls), mine[k]))
            if ws == 1:
                ckpts[cls][scene_id] = True                                               # P:580-581
                write_scene_checkpoint("projection_2d_to_3d", cls, ckpts[cls])
        out = res.to_rle_dict() if os.environ.get("BFF_SAVE_RLE") == "1" and not res.debug.get("empty_form") else res.to_dict()
        save_result(out, cfg.mask_3d_dir, cls, scene_id)                                    # P:630-634

    project_classes_stream(items, cfg, device, consume, n_loaders=int(os.environ.get("BFF_LOADERS", "2")))
    if ws > 1:
        # one reduction of the (class, scene) completion flags; rank 0 alone writes every class's checkpoint
        flags = torch.zeros((len(classes), max(len(scene_ids), 1)), dtype=torch.int32, device=_coll_device(device))
        if done:
            idx = torch.tensor(done, dtype=torch.long)
            flags[idx[:, 0], idx[:, 1]] = 1
        dist.reduce(flags, dst=0, op=dist.ReduceOp.SUM)
        if rank == 0:
            got = flags.cpu()
            for ci, c in enumerate(classes):
                for i in torch.nonzero(got[ci]).view(-1).tolist():
                    ckpts[c][scene_ids[i]] = True
                write_scene_checkpoint("projection_2d_to_3d", c, ckpts[c])
        _finish_ranks()
    return 0


def _clip_available():
    try:
        import clip  # noqa: F401
        return True
    except ImportError:
        return False


def _text_encoder(path, device="cuda"):
    """CLIP ViT-L/14 text encoder (R:147) when the `clip` package is importable; otherwise a file of
    precomputed text embeddings {text: (D,) tensor} given by BFF_TEXT_EMBEDDINGS."""
    if path:
        table = torch.load(path, weights_only=True)
        return lambda text: table[text].reshape(1, -1)
    import clip                                                                         # noqa: F401
    dev = device if torch.cuda.is_available() else "cpu"
    model, _ = clip.load("ViT-L/14", device=dev)

    def enc(text):
        with torch.no_grad():
            return model.encode_text(clip.tokenize([text]).to(dev))
    return enc


def refinement_main(argv=None):
    """python tools/refinement.py --config configs/config.yaml --cls "<class>"            (R:135-428)"""
    args = _parser("Beyond-Fixed-Forms refinement (MI355X)").parse_args(argv)
    rc = launch_ranks(argv)
    if rc is not None:
        return rc
    cfg = load_config(args.config)
    _lib.load()
    _host_threads()
    cls = args.cls
    from .distributed import ClassBatch, shard_scenes
    rank, ws, device = init_ranks()
    ckpt = read_scene_checkpoint("refinement", cls)
    # BFF_TEXT_BANK=<file>: similarity service persisted by an earlier run (bank of the 198 labels + queries);
    # created on first use, so the CLIP text encoder runs once per label ever, not twice per matched mask
    bank_file = os.environ.get("BFF_TEXT_BANK")
    emb_file = os.environ.get("BFF_TEXT_EMBEDDINGS")
    if bank_file and os.path.exists(bank_file):
        need_enc = emb_file or _clip_available()
        sim = TextSimilarity.from_file(bank_file, device, _text_encoder(emb_file, device) if need_enc else None)
    else:
        sim = TextSimilarity(_text_encoder(emb_file, device), device)
    stage2_dir = os.path.join(cfg.mask_3d_dir, cls)
    ids = [s.replace(".pth", "") for s in sorted(s for s in os.listdir(stage2_dir) if s.endswith("_00.pth"))]   # R:154
    p1 = lambda sid: os.path.join(cfg.stage_1_results_dir, f"{sid}.pth")
    p2 = lambda sid: os.path.join(stage2_dir, f"{sid}.pth")
    have = [os.path.exists(p1(sid)) and os.path.exists(p2(sid)) for sid in ids]             # R:175-178
    # A scene without its stage-1 file is skipped by pass 1 only (R:178), which shifts the reference's per-scene lists
    # against its scene loop in pass 2 (R:330): that order dependence is reproduced by keeping such a class on one rank.
    owners = ws if all(have) else 1
    mine = shard_scenes(ids, rank, owners) if rank < owners else []
    s_max = max(1, -(-len(ids) // owners))
    batch = ClassBatch(cfg, cls, sim, device, ids, s_max)
    for i in mine:
        if have[i]:
            # user data files written by Open3DIS / by the projection stage (R:182-183)
            batch.add(ids[i], torch.load(p1(ids[i]), map_location="cpu", weights_only=False),
                      torch.load(p2(ids[i]), map_location="cpu", weights_only=False))
        else:
            batch.add(ids[i], None, None)
    batch.finish()
    if bank_file and rank == 0:
        sim.save(bank_file)
    if rank == 0:
        res = batch.results()                                   # all scenes of the class (gathered over RCCL when ws > 1)
        for scene_id in ids:
            if scene_id not in res:
                continue
            fr = res[scene_id]
            d = fr.to_rle_dict() if os.environ.get("BFF_SAVE_RLE") == "1" else fr.to_dict()
            d = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}           # reference saves CPU tensors
            save_result(d, cfg.final_output_dir, cls, scene_id)                             # R:422-426
            if fr.rows is not None and len(fr.final_class):
                ckpt[scene_id] = True                                                       # R:427-428
                write_scene_checkpoint("refinement", cls, ckpt)
    if ws > 1:
        _finish_ranks()
    return 0


def _reproject_parser():
    p = _stage_parser("Beyond-Fixed-Forms 3D->2D reprojection: a class's instances as 2-D masks of the colour frames (MI355X)")
    p.add_argument("--every", type=int, default=None,
                   help="Render into every n-th colour frame (default: downsample_ratio, the frames the 2-D stage saw)")
    return p


def _saved_instances(result, n_points, device):
    """A saved stage file {"ins", "conf", "final_class"} -> what reproject.instance_masks_2d reads: bit rows on the
    device, confidences, class strings (the reference's list-valued empty forms give no rows)."""
    from types import SimpleNamespace
    ins, classes = result["ins"], result["final_class"]
    classes = [str(c) for c in (classes.reshape(-1).tolist() if torch.is_tensor(classes) else classes)]
    if isinstance(ins, (list, tuple)) and len(ins) and isinstance(ins[0], dict):
        from .scene import runs_from_rles
        if any(int(r["length"]) != n_points for r in ins):
            raise ValueError("RLE instances of another length than the cloud")
        t = lambda a: torch.from_numpy(a).to(device)
        rows = _lib.rle_to_rows(*[t(a) for a in runs_from_rles(ins, "instance")], n_points)
    else:
        ins = torch.as_tensor(ins)
        if ins.dim() != 2 or ins.shape[0] == 0 or ins.shape[1] != n_points or not classes:
            return SimpleNamespace(rows=None, conf=[], final_class=[])
        rows = _lib.pack_rows((ins.to(device) == 1).contiguous())
    return SimpleNamespace(rows=rows, conf=result["conf"], final_class=classes)


def reproject_main(argv=None):
    """python tools/reproject_3d_to_2d.py --config configs/config.yaml --cls "<class>" [--stage final|mask_3d] [--every n]
    For every scene of the class's output directory: its instances rendered into every n-th colour frame
    (reproject.instance_masks_2d) and saved to reprojected_2d_dir/<cls>/<scene>.pth in the mask_2d file format (RLE
    dicts).  Only the intrinsics, the poses and the cloud are read -- no depth frame."""
    from types import SimpleNamespace

    from . import masks2d, reproject
    from .io import read_matrix_txt
    from .scene import viewed_frame_ids
    args = _reproject_parser().parse_args(argv)
    cfg = load_config(args.config)
    cls = args.cls
    data_path = os.path.join(cfg.final_output_dir if args.stage == "final" else cfg.mask_3d_dir, cls)
    if not os.path.isdir(data_path):
        print(f"no {args.stage} output for class {cls!r}: {data_path} is not a directory", file=sys.stderr)
        return 1
    out_dir = cfg.get("reprojected_2d_dir")
    if not out_dir:
        raise ValueError("reprojected_2d_dir is not set in the config")
    every = int(cfg.downsample_ratio) if args.every is None else int(args.every)
    if every < 1:
        raise ValueError(f"--every must be >= 1, got {every}")
    _lib.load()
    _host_threads()
    device = "cuda"
    for name in sorted(s for s in os.listdir(data_path) if s.endswith(".pth")):
        scene_id = name[:-4]
        print("Working on", scene_id, "class", cls)
        scene_dir = os.path.join(cfg.scene_2d_dir, scene_id)
        color_dir = os.path.join(scene_dir, "color")
        color_files = [f for f in os.listdir(color_dir) if f.endswith(".jpg")] if os.path.isdir(color_dir) else []
        frame_ids = viewed_frame_ids(color_files, every)
        scene = SimpleNamespace(scene_id=scene_id, points=np.load(os.path.join(cfg.scene_npy_dir, f"{scene_id}.npy")),
                                cam_intr=read_matrix_txt(os.path.join(scene_dir, "intrinsic", "intrinsic_color.txt")),
                                poses={f: read_matrix_txt(os.path.join(scene_dir, "pose", f"{f}.txt")) for f in frame_ids})
        geom = reproject.geometry_for_frames(scene, cfg, frame_ids, device)
        # the stage's own output file, written by this project's scripts or the reference's (a pickled dict of tensors)
        result = torch.load(os.path.join(data_path, name), map_location="cpu", weights_only=False)
        masks = reproject.instance_masks_2d(geom, frame_ids, _saved_instances(result, geom.n_points, device), cfg)
        save_result(masks2d.encode_2d_masks(masks), out_dir, cls, scene_id)
    return 0


def _stage_main(parser, argv, dir_keys, check, scene):
    """What split_main, cluster_main, snap_main and lift_main share.  dir_keys: the config's directories the stage needs,
    its output directory first; check(cfg): the stage's config values, so that a bad one stops the run before the first
    scene; scene(cfg, scene_id, result, device): the saved file of one scene -> (its instances with the rows replaced,
    the length of their cloud), or None for a file that passes through as it is (the reference's empty forms).  The new
    instances are saved in the stage's own file format, with the attribute `parent`, where the stage sets one, under the
    added key "parent"."""
    args = parser.parse_args(argv)
    cfg = load_config(args.config)
    cls = args.cls
    data_path = os.path.join(cfg.final_output_dir if args.stage == "final" else cfg.mask_3d_dir, cls)
    if not os.path.isdir(data_path):
        print(f"no {args.stage} output for class {cls!r}: {data_path} is not a directory", file=sys.stderr)
        return 1
    for key in dir_keys:
        if not cfg.get(key):
            raise ValueError(f"{key} is not set in the config")
    out_dir = cfg.get(dir_keys[0])
    check(cfg)
    _lib.load()
    _host_threads()
    device = "cuda"
    for name in sorted(s for s in os.listdir(data_path) if s.endswith(".pth")):
        scene_id = name[:-4]
        print("Working on", scene_id, "class", cls)
        # the stage's own output file, written by this project's scripts or the reference's (a pickled dict of tensors)
        result = torch.load(os.path.join(data_path, name), map_location="cpu", weights_only=False)
        done = scene(cfg, scene_id, result, device)
        if done is None:
            save_result(result, out_dir, cls, scene_id)
            continue
        inst, n_points = done
        ins = _lib.rows_to_rle(inst.rows, n_points) if os.environ.get("BFF_SAVE_RLE") == "1" else \
            _lib.unpack_rows(inst.rows, n_points).cpu()
        out = {"ins": ins, "conf": inst.conf.cpu() if torch.is_tensor(inst.conf) else inst.conf, "final_class": inst.final_class}
        if hasattr(inst, "parent"):
            out["parent"] = inst.parent
        save_result(out, out_dir, cls, scene_id)
    return 0


def _scene_cloud(cfg, scene_id, **kw):
    return np.load(os.path.join(cfg.scene_npy_dir, f"{scene_id}.npy"), **kw)


def _split_parser():
    return _stage_parser("Beyond-Fixed-Forms 3-D instances split into spatially connected parts (MI355X)")


def split_main(argv=None):
    """python tools/split_instances_3d.py --config configs/config.yaml --cls "<class>" [--stage final|mask_3d]
    For every scene of the class's output directory: the cloud binned into a voxel grid of split_voxel metres once, every
    instance cut into its connected parts (spatial.split_instances) and saved to split_output_dir/<cls>/<scene>.pth in the
    stage's own file format, with the parts' parent instances under the added key "parent".  Only the cloud is read."""
    from . import spatial

    def scene(cfg, scene_id, result, device):
        grid = spatial.voxel_grid(_scene_cloud(cfg, scene_id), spatial.split_voxel(cfg), device)
        inst = _saved_instances(result, grid.n_points, device)
        return None if inst.rows is None else (spatial.split_instances(grid, inst, cfg), grid.n_points)

    check = lambda cfg: (spatial.split_voxel(cfg), spatial.split_min_points(cfg), spatial.split_mode(cfg))
    return _stage_main(_split_parser(), argv, ("split_output_dir",), check, scene)


def _cluster_parser():
    return _stage_parser("Beyond-Fixed-Forms 3-D instances clustered by density, DBSCAN with a deterministic border rule (MI355X)")


def cluster_main(argv=None):
    """python tools/cluster_instances_3d.py --config configs/config.yaml --cls "<class>" [--stage final|mask_3d]
    For every scene of the class's output directory: the search index of the cloud at cluster_eps metres built once, every
    instance cut into its density clusters (density.cluster_instances: noise dropped) and saved to
    cluster_output_dir/<cls>/<scene>.pth in the stage's own file format, with the clusters' parent instances under the
    added key "parent".  Only the cloud is read."""
    from . import density

    def scene(cfg, scene_id, result, device):
        index = density.density_index(_scene_cloud(cfg, scene_id), density.cluster_eps(cfg), device)
        inst = _saved_instances(result, index.n_points, device)
        return None if inst.rows is None else (density.cluster_instances(index, inst, cfg), index.n_points)

    check = lambda cfg: (density.cluster_eps(cfg), density.cluster_min_samples(cfg), density.cluster_min_points(cfg),
                         density.cluster_mode(cfg))
    return _stage_main(_cluster_parser(), argv, ("cluster_output_dir",), check, scene)


def _snap_parser():
    return _stage_parser("Beyond-Fixed-Forms 3-D instances snapped to superpoints (MI355X)")


def snap_main(argv=None):
    """python tools/snap_instances_3d.py --config configs/config.yaml --cls "<class>" [--stage final|mask_3d]
    For every scene of the class's output directory: the index of superpoint_dir/<scene>.pth built once, every instance
    snapped to the superpoints it holds snap_ratio of (superpoints.snap_instances) and saved to
    snap_output_dir/<cls>/<scene>.pth in the stage's own file format, with the surviving rows' input instances under the
    added key "parent".  Only the cloud's length and the superpoint file are read."""
    from . import superpoints

    def scene(cfg, scene_id, result, device):
        n_points = int(_scene_cloud(cfg, scene_id, mmap_mode="r").shape[0])
        # the dataset's own file: an ndarray or a tensor of ids (scannet_loader.py:92 accepts both)
        spp = torch.load(os.path.join(cfg.get("superpoint_dir"), f"{scene_id}.pth"), map_location="cpu", weights_only=False)
        n_ids = int(spp.numel()) if torch.is_tensor(spp) else int(np.asarray(spp).size)
        if n_ids != n_points:
            raise ValueError(f"{scene_id}: a superpoint file of {n_ids} ids for a cloud of {n_points} points")
        index = superpoints.superpoint_index(spp, device)
        inst = _saved_instances(result, n_points, device)
        return None if inst.rows is None else (superpoints.snap_instances(index, inst, cfg), n_points)

    check = lambda cfg: (superpoints.snap_ratio(cfg), superpoints.snap_mode(cfg), superpoints.snap_min_points(cfg))
    return _stage_main(_snap_parser(), argv, ("snap_output_dir", "superpoint_dir"), check, scene)


def _subsample_parser():
    p = argparse.ArgumentParser(description="Beyond-Fixed-Forms voxel subsample of the scene clouds (MI355X)")
    p.add_argument("--config", type=str, required=True, help="Config")
    p.add_argument("--scene", type=str, action="append", default=None,
                   help="A scene id (repeatable); without it every <scene>.npy of scene_npy_dir")
    return p


def subsample_main(argv=None):
    """python tools/subsample_cloud.py --config configs/config.yaml [--scene <id> ...]
    For every scene_npy_dir/<scene>.npy (or the named ones): one point of every cell of subsample_voxel metres
    (lift.subsample), saved as subsample_npy_dir/<scene>.npy -- those rows of the file, all columns, dtype kept -- with
    the kept indices (int32) in subsample_npy_dir/sample/<scene>.npy.  A second config whose scene_npy_dir names that
    folder runs the projection stage unchanged on the small clouds."""
    from . import lift
    args = _subsample_parser().parse_args(argv)
    cfg = load_config(args.config)
    out_dir = cfg.get("subsample_npy_dir")
    if not out_dir:
        raise ValueError("subsample_npy_dir is not set in the config")
    voxel = lift.subsample_voxel(cfg)                                    # a bad value stops the run before the first scene
    src_dir = cfg.get("scene_npy_dir")
    if not src_dir or not os.path.isdir(src_dir):
        print(f"no clouds: scene_npy_dir {src_dir!r} is not a directory", file=sys.stderr)
        return 1
    if os.path.abspath(out_dir) == os.path.abspath(src_dir):
        raise ValueError("subsample_npy_dir is scene_npy_dir itself: the clouds would be overwritten")
    scenes = args.scene if args.scene else sorted(s[:-4] for s in os.listdir(src_dir) if s.endswith(".npy"))
    _lib.load()
    _host_threads()
    os.makedirs(os.path.join(out_dir, "sample"), exist_ok=True)
    for scene_id in scenes:
        points = np.load(os.path.join(src_dir, f"{scene_id}.npy"))
        sample = lift.subsample(points, voxel, "cuda").cpu().numpy()
        print("Working on", scene_id, ":", len(sample), "of", points.shape[0], "points")
        np.save(os.path.join(out_dir, f"{scene_id}.npy"), points[sample])
        np.save(os.path.join(out_dir, "sample", f"{scene_id}.npy"), sample)
    return 0


def _lift_parser():
    return _stage_parser("Beyond-Fixed-Forms 3-D instances lifted from a subsampled cloud to the full cloud (MI355X)")


def _saved_mask_length(result):
    """The point count the masks of a saved stage file were made for, None for the reference's empty forms."""
    ins = result["ins"]
    if isinstance(ins, (list, tuple)):
        return int(ins[0]["length"]) if len(ins) and isinstance(ins[0], dict) else None
    ins = torch.as_tensor(ins)
    return int(ins.shape[1]) if ins.dim() == 2 and ins.shape[0] > 0 and ins.shape[1] > 0 else None


def lift_main(argv=None):
    """python tools/lift_instances_3d.py --config configs/config.yaml --cls "<class>" [--stage final|mask_3d]
    The config is the small run's.  For every scene of the class's output directory: the search index of the small cloud
    (scene_npy_dir/<scene>.npy) built once, one search for the points of the full cloud (lift_target_npy_dir/<scene>.npy)
    within lift_max_dist, every instance lifted (lift.lift_instances) and saved to lift_output_dir/<cls>/<scene>.pth in
    the stage's own file format, the masks of the full cloud's length.  Only the two clouds are read."""
    from . import lift

    def scene(cfg, scene_id, result, device):
        length = _saved_mask_length(result)
        if length is None:
            return None
        source = _scene_cloud(cfg, scene_id)
        target = np.load(os.path.join(cfg.get("lift_target_npy_dir"), f"{scene_id}.npy"))
        n_source, n_target = int(source.shape[0]), int(target.shape[0])
        if length != n_source:
            raise ValueError(f"{scene_id}: masks of {length} points for a source cloud of {n_source} points")
        inst = _saved_instances(result, n_source, device)
        if inst.rows is None:
            return None
        nn = lift.nearest(lift.nearest_index(source, lift.lift_max_dist(cfg), device), target)
        return lift.lift_instances(nn, inst, n_source, n_target), n_target     # the rows keep their order: no `parent`

    return _stage_main(_lift_parser(), argv, ("lift_output_dir", "lift_target_npy_dir"), lift.lift_max_dist, scene)


def _assemble_parser():
    p = argparse.ArgumentParser(description="Beyond-Fixed-Forms: a scene's prediction assembled from all of its query "
                                            "classes, with 3-D mask NMS (MI355X)")
    p.add_argument("--config", type=str, required=True, help="Config")
    which = p.add_mutually_exclusive_group(required=True)
    which.add_argument("--cls", type=str, action="append", help="A class (repeatable); their order is the class index")
    which.add_argument("--all-classes", action="store_true", help="Every sub-directory of the stage's directory, sorted")
    p.add_argument("--stage", type=str, default="final", choices=("final", "mask_3d"),
                   help="Whose instances: the refinement's (final_output_dir) or the projection stage's (mask_3d_dir)")
    p.add_argument("--point-labels", action="store_true",
                   help="Also save point_instance (0 = none, else 1 + row) and point_semantic (class position, -1 = none)")
    return p


def assembled_dict(assembled, rle=False, point_labels=False):
    """What assemble_main saves for one scene: the stage's file format ("ins" dense bool rows or, with rle, RLE dicts; "conf";
    "final_class") plus "classes", "source" (int64 [R][2]: class position and row of every instance in its class's file) and
    "removed_by"; with point_labels also "point_instance" and "point_semantic".  A scene without any row: the reference's
    empty form with the same added keys."""
    from . import assemble
    r = int(assembled.rows.shape[0])
    if r == 0:
        out = {"ins": [], "conf": [], "final_class": []}
    else:
        ins = _lib.rows_to_rle(assembled.rows, assembled.n_points) if rle else \
            _lib.unpack_rows(assembled.rows, assembled.n_points).cpu()
        out = {"ins": ins, "conf": assembled.conf, "final_class": list(assembled.final_class)}
    out["classes"] = list(assembled.classes)
    out["source"] = torch.stack([assembled.source_class, assembled.source_row], dim=1)
    out["removed_by"] = assembled.removed_by
    if point_labels:
        instance, semantic = assemble.point_labels(assembled)
        out["point_instance"], out["point_semantic"] = instance.cpu(), semantic.cpu()
    return out


def assemble_main(argv=None):
    """python tools/assemble_scene_3d.py --config configs/config.yaml (--cls a --cls b ... | --all-classes)
                                          [--stage final|mask_3d] [--point-labels]
    Scenes = the union of the classes' <scene>.pth names; a class without the scene contributes nothing.  Every scene's
    rows of all classes become one set of instances (assemble.assemble_scene: NMS by score, optionally exclusive, small
    ones dropped) saved to assembled_output_dir/<scene>.pth in the stage's file format.  Only the cloud's length is read."""
    from . import assemble
    args = _assemble_parser().parse_args(argv)
    cfg = load_config(args.config)
    stage_dir = cfg.final_output_dir if args.stage == "final" else cfg.mask_3d_dir
    if not os.path.isdir(stage_dir):
        print(f"no {args.stage} output: {stage_dir} is not a directory", file=sys.stderr)
        return 1
    if args.all_classes:
        classes = sorted(c for c in os.listdir(stage_dir) if os.path.isdir(os.path.join(stage_dir, c)))
    else:
        classes = list(dict.fromkeys(args.cls))
    missing = [c for c in classes if not os.path.isdir(os.path.join(stage_dir, c))]
    if missing or not classes:
        print(f"no {args.stage} output for {missing if missing else 'any class'} under {stage_dir}", file=sys.stderr)
        return 1
    out_dir = cfg.get("assembled_output_dir")
    if not out_dir:
        raise ValueError("assembled_output_dir is not set in the config")
    assemble.check_config(cfg)                                   # a bad value stops the run before the first scene
    lists = {c: {s for s in os.listdir(os.path.join(stage_dir, c)) if s.endswith(".pth")} for c in classes}
    _lib.load()
    _host_threads()
    device = "cuda"
    os.makedirs(out_dir, exist_ok=True)
    for name in sorted(set().union(*lists.values())):
        scene_id = name[:-4]
        print("Working on", scene_id, ":", sum(name in lists[c] for c in classes), "classes")
        n_points = int(_scene_cloud(cfg, scene_id, mmap_mode="r").shape[0])
        # the stage's own output files, written by this project's scripts or the reference's (pickled dicts of tensors)
        # (a class without the scene stands in as the empty form, so that class positions are those of the run's list)
        results = {c: torch.load(os.path.join(stage_dir, c, name), map_location="cpu", weights_only=False)
                   if name in lists[c] else {"ins": [], "conf": [], "final_class": []} for c in classes}
        got = assemble.assemble_scene(results, n_points, cfg, device)
        torch.save(assembled_dict(got, os.environ.get("BFF_SAVE_RLE") == "1", args.point_labels),
                   os.path.join(out_dir, f"{scene_id}.pth"))
    return 0


def _select_views_parser():
    p = argparse.ArgumentParser(description="Beyond-Fixed-Forms: the frames that see each 3-D instance best, and the boxes to "
                                            "crop it with (MI355X)")
    p.add_argument("--config", type=str, required=True, help="Config")
    p.add_argument("--cls", type=str, default=None, help="Class (not needed with --assembled)")
    p.add_argument("--stage", type=str, default="final", choices=("final", "mask_3d"),
                   help="Whose instances: the refinement's (final_output_dir) or the projection stage's (mask_3d_dir)")
    p.add_argument("--every", type=int, default=None,
                   help="Look at every n-th colour frame (default: downsample_ratio, the frames the 2-D stage saw)")
    p.add_argument("--assembled", action="store_true",
                   help="The scenes' assembled predictions (assembled_output_dir/<scene>.pth) instead of one class's files")
    return p


def select_views_main(argv=None):
    """python tools/select_views_3d.py --config configs/config.yaml --cls "<class>" [--stage final|mask_3d] [--every n]
                                        [--assembled]
    For every scene of the class's output directory (with --assembled: of assembled_output_dir): per instance, the points
    every n-th colour frame's depth confirms, their pixel box, the views_top_k best frames and their crops
    (views.scene_views), saved to views_output_dir/<cls>/<scene>.pth (with --assembled: views_output_dir/<scene>.pth).
    The depth frames are read, or rendered as depth_from_cloud / depth_from_mesh say."""
    from . import views
    from .io import load_scene_frames
    from .scene import geometry_for_depth_frames
    parser = _select_views_parser()
    args = parser.parse_args(argv)
    if not args.assembled and not args.cls:
        parser.error("--cls is required without --assembled")
    cfg = load_config(args.config)
    cls = "" if args.assembled else args.cls
    if args.assembled:
        data_path = cfg.get("assembled_output_dir")
        if not data_path:
            raise ValueError("assembled_output_dir is not set in the config")
    else:
        data_path = os.path.join(cfg.final_output_dir if args.stage == "final" else cfg.mask_3d_dir, cls)
    if not os.path.isdir(data_path):
        what = "assembled output" if args.assembled else f"{args.stage} output for class {cls!r}"
        print(f"no {what}: {data_path} is not a directory", file=sys.stderr)
        return 1
    out_dir = cfg.get("views_output_dir")
    if not out_dir:
        raise ValueError("views_output_dir is not set in the config")
    views.check_config(cfg)                                      # a bad value stops the run before the first scene
    every = int(cfg.downsample_ratio) if args.every is None else int(args.every)
    if every < 1:
        raise ValueError(f"--every must be >= 1, got {every}")
    _lib.load()
    _host_threads()
    device = "cuda"
    on_dev = os.environ.get("BFF_DEPTH_ON_DEVICE") == "1"
    for name in sorted(s for s in os.listdir(data_path) if s.endswith(".pth")):
        scene_id = name[:-4]
        print("Working on", scene_id, "assembled" if args.assembled else f"class {cls}")
        scene = load_scene_frames(cfg, scene_id, every, depth_on_device=on_dev)
        geom = geometry_for_depth_frames(scene, cfg, list(scene.poses), device)
        # the stage's own output file, written by this project's scripts or the reference's (a pickled dict of tensors)
        result = torch.load(os.path.join(data_path, name), map_location="cpu", weights_only=False)
        out = views.scene_views(geom, _saved_instances(result, geom.n_points, device), cfg)
        save_result(out, out_dir, cls, scene_id)                 # cls "": views_output_dir/<scene>.pth
    return 0


def _evaluation_parser():
    """eval_scannet200.py:29-32 plus what the reference hard-codes (:74-76) or imports from its dataset tables."""
    p = argparse.ArgumentParser(description="Beyond-Fixed-Forms per-class evaluation (MI355X)")
    p.add_argument("--cls", type=str, required=True, help="Specific class to evaluate")
    p.add_argument("--config", type=str, default="configs/config.yaml", help="Config (final_output_dir is read from it)")
    p.add_argument("--gt-dir", type=str, default="./data/Scannet200/Scannet200_3D/groundtruth",
                   help="Directory of the ground-truth <scene>.pth files")
    p.add_argument("--results-file", type=str, default="./evaluation/eval_results/overall_results.txt",
                   help="Summary file whose line of this class is replaced")
    p.add_argument("--label-table", type=str, required=True,
                   help='JSON {"class_labels": [...], "semantic_ids": [...]}: the evaluator\'s class names and the '
                        "dataset's raw semantic id of each")
    p.add_argument("--assembled", action="store_true",
                   help="Score the scenes' assembled predictions (assembled_output_dir/<scene>.pth, every class in one file) "
                        "instead of final_output_dir/<cls>")
    p.add_argument("--use-conf", action="store_true",
                   help="Rank the predictions by the files' confidences instead of the reference's 1.0 for each")
    return p


def evaluation_main(argv=None):
    """python tools/eval_scannet200.py --cls "<class>" --label-table labels.json [--assembled] [--use-conf]
    (eval_scannet200.py:70-148)  The class's final files against the ground truth: AP, AP50, AP25 and the recalls of the
    class into its line of the results file, every label's into result.txt beside it.  --assembled: the scenes' assembled
    files (assemble_main), every class in one file, instead -- all scenes of assembled_output_dir are scored, so a class's
    values equal its own run's where it has a file for each of them; --use-conf: the files' confidences instead of 1.0."""
    import json

    from . import evaluation as ev
    args = _evaluation_parser().parse_args(argv)
    cfg = load_config(args.config)
    with open(args.label_table, "r") as f:
        table = json.load(f)
    # semantic_ids is the dataset's whole list (BENCHMARK_SEMANTIC_IDXS: 200 ids, wall and floor first); the evaluator's
    # `- 2 + 1` for scannet200 (EVAL:272-273) is what lines position p of it up with class_labels[p - 2]
    labels, semantic_ids = list(table["class_labels"]), list(table["semantic_ids"])
    cls = args.cls
    data_path = cfg.get("assembled_output_dir") if args.assembled else os.path.join(cfg.final_output_dir, cls)
    if args.assembled and not data_path:
        raise ValueError("assembled_output_dir is not set in the config")
    if not os.path.isdir(data_path):
        what = "assembled output" if args.assembled else f"final output for class {cls!r}"
        print(f"no {what}: {data_path} is not a directory", file=sys.stderr)
        return 1
    _lib.load()
    _host_threads()
    device = "cuda"
    evaluator = ev.Evaluator(labels, device=device)
    for scene in sorted(s for s in os.listdir(data_path) if s.endswith(".pth")):            # :77
        loader = torch.load(os.path.join(args.gt_dir, scene), map_location="cpu", weights_only=False)
        sem_gt = ev.semantic_positions(loader[2], semantic_ids)                             # :88-97
        truth = evaluator.prepare_ground_truth(sem_gt, np.asarray(loader[3]).astype(np.int32))
        result = torch.load(os.path.join(data_path, scene), map_location="cpu", weights_only=False)
        preds, rows = ev.final_file_predictions(result, scene.replace(".pth", ""), labels, truth.n_points, device)
        if args.use_conf:
            conf = result["conf"]
            conf = conf.reshape(-1).tolist() if torch.is_tensor(conf) else list(conf)
            if len(conf) != len(preds):
                raise ValueError(f"{scene}: {len(preds)} instances and {len(conf)} confidences")
            for pred, c in zip(preds, conf):
                pred["conf"] = float(c)
        evaluator.add_scan(preds, ground_truth=truth, pred_rows=rows)
    avgs = evaluator.evaluate()
    results_dir = os.path.dirname(os.path.abspath(args.results_file))
    os.makedirs(results_dir, exist_ok=True)
    ev.write_result_file(avgs, evaluator.eval_class_labels, os.path.join(results_dir, "result.txt"))   # EVAL:597
    if cls not in avgs["classes"]:
        raise KeyError(f"class {cls!r} is not in the label table")                         # :142
    print(ev.format_results(avgs, [cls]), end="")
    ev.update_results_file(args.results_file, cls, [avgs["classes"][cls][k] for k in
                                                    ("ap", "ap50%", "ap25%", "rc", "rc50%", "rc25%")], labels)
    return 0
