"""Scenes in flight on several streams: the scene lists, the runners and the child-process worker of test_gpu_pipelined.py.

One list of small scenes of mixed shapes that between them take every path of the scene call (fast, re-issued with the
large group tables, general from workspace views, step by step, sensor depth, a workspace that grows) is run the way
bench.py runs its timed loop -- `scene_streams`, `_lib.on_stream`, `projection_front` / `projection_back` through
`pipeline.pipelined`, a `ClassBatch` fed in the back half -- and through `project_stream` / `project_classes_stream`.
Everything a run delivers is flattened into a dict of NumPy arrays (`s<j>.*` stage 2 of list entry j, `f<j>.*` its
final result), so that runs, the one-at-a-time reference, the oracle and the children's .npz files compare key by key.

Run as a script (`python tests/pipelined_case.py OUT.npz [SCENES.pt]`) this file is the worker of the stream-switch test:
BFF_HEAVY_STREAMS and BFF_AUX_STREAM are read once per process, so each value gets a fresh child."""
import copy
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
QUERY = "table"
DELAY_CAP_MS = 100.0

G325 = dict(shape="tiny", seed=30, n_labels=50, n_masks=64, n_views=24, cut_masks=False)
G552 = dict(shape="tiny", seed=30, n_labels=90, n_masks=64, n_views=40, cut_masks=False)
# name -> (make_scene keywords, variant, the path the scene call must take)
SCENES = {
    "tiny31": (dict(shape="tiny", seed=31), None, "fast"),
    "u64": (dict(shape="tiny", seed=32, n_points=4001, n_masks=40), None, "fast"),      # 64-bit mask words, ragged nw
    "c1": (dict(shape="c1", seed=33), None, "fast"),                                     # the workspace grows
    "g325": (G325, None, "fast"),                 # 325 groups: issued again with the 512 tables inside collect
    "g552": (G552, None, "general"),              # 552 groups: the general path from views of the workspace
    "nomask": (dict(shape="tiny", seed=34), "no_masks", "step"),
    # nine views: as in every other scene here, two of its distinct filter values then share one of the 64 hash partitions
    # of the value set, so a set shrunk to one value per partition overflows (with the default six views none do)
    "sensor": (dict(shape="tiny", seed=35, n_views=9), "sensor_depth", "fast"),
    "tiny33": (dict(shape="tiny", seed=33), None, "fast"),
}
# 2 * PIPELINE_DEPTH + 2 entries; with four streams every workspace meets three different shapes, the last two entries
# come back to scenes whose DeviceScene remembers its group capacity
MIXED = ["tiny31", "u64", "c1", "g325", "g552", "nomask", "sensor", "tiny33", "g325", "tiny31"]
SAME_SIZED = [n for n in MIXED if n != "c1"]      # one image size, hence one config: what project_stream takes


def eid(j):
    return f"e{j:02d}"


class Case:
    """The host side every run shares: the scenes, their configs, the text bank."""

    def __init__(self, scenes_file=None):
        """scenes_file: the scenes as another process built and saved them (`save_scenes`; generating the two
        64-mask scenes takes longer than everything a child does with them)."""
        from beyond_fixed_forms_amd.config import Config
        from beyond_fixed_forms_amd.synthetic import make_scene, make_text_bank, with_sensor_depth
        from oracle.make_golden_shared import bank_encoder
        self.scenes, self.cfgs = {}, {}
        saved = torch.load(scenes_file, weights_only=False) if scenes_file else {}
        for name, (kw, variant, _path) in SCENES.items():
            if saved:
                sc = saved[name]
            else:
                sc = make_scene(**kw)
                if variant == "no_masks":
                    sc.mask_2d = []
                elif variant == "sensor_depth":
                    sc = with_sensor_depth(sc)
            sc.scene_id = name
            self.scenes[name] = sc
            self.cfgs[name] = Config.with_defaults(width_2d=sc.width, height_2d=sc.height)
        bank, index = make_text_bank(64, seed=3)
        self.enc = bank_encoder(bank, index)            # float16 embeddings, as CLIP on a GPU
        self._sim = None

    def save_scenes(self, path):
        torch.save(self.scenes, path)

    def sim(self):
        if self._sim is None:
            from beyond_fixed_forms_amd.refinement import TextSimilarity
            self._sim = TextSimilarity(self.enc, DEV)
        return self._sim

    def class_cfg(self, names):
        return self.cfgs[names[0]]                      # the refinement reads no image size

    def devices(self, names):
        """Fresh DeviceScene + DeviceStage1 of every distinct scene of `names` (an entry that comes back meets the
        object of its first visit, with whatever that visit remembered on it)."""
        from beyond_fixed_forms_amd.refinement import prepare_stage1
        from beyond_fixed_forms_amd.scene import prepare_scene
        out = {}
        for name in dict.fromkeys(names):
            sc = self.scenes[name]
            out[name] = (prepare_scene(sc, self.cfgs[name], device=DEV), prepare_stage1(sc.stage1, DEV))
        return out

    def oracle_scene(self, name):
        """The scene as the oracle takes it: sensor depth resized on the host (io.resize_bilinear_f32)."""
        sc = self.scenes[name]
        if getattr(sc, "depths_raw", None) is not None and not sc.depths:
            from beyond_fixed_forms_amd.io import resize_bilinear_f32
            host = copy.copy(sc)
            host.depths = {f: resize_bilinear_f32(m.astype(np.float32) / np.float32(1000), sc.width, sc.height)
                           for f, m in sc.depths_raw.items()}
            host.depths_raw = None
            return host
        return sc


# ------------------------------------------------------------------ what a run delivers, as arrays
def groups_arrays(groups):
    lists = [list(g) for g in groups]
    offs = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(g) for g in lists], out=offs[1:])
    return offs, np.asarray([m for g in lists for m in g], dtype=np.int64)


def strings(items):
    return np.asarray(list(items), dtype=str) if len(items) else np.zeros(0, dtype="<U1")


def stage2_arrays(res, had_prefetch):
    offs, members = groups_arrays(res.groups)
    return {"rows": res.rows.cpu().numpy(), "conf": res.conf.cpu().numpy(), "final_class": strings(res.final_class),
            "empty": np.asarray(bool(res.debug.get("empty_form", False))),
            "path": np.asarray(res.debug.get("path", "step").split(" ")[0]),
            "goffs": offs, "gmembers": members, "prefetch": np.asarray(bool(had_prefetch))}


def final_arrays(f):
    if f.rows is None:
        return {"lists": np.asarray(True), "rows": np.zeros((0, 0), np.int64), "conf": np.zeros(0, np.float32),
                "final_class": strings(f.final_class)}
    return {"lists": np.asarray(False), "rows": f.rows.cpu().numpy(), "conf": torch.as_tensor(f.conf).cpu().numpy(),
            "final_class": strings(f.final_class)}


def pack_bits(dense):
    """bool (R, N) -> the int64 [R][nw] bit rows the device path keeps (bit p of word p // 64)."""
    r, n = dense.shape
    nw = (n + 63) // 64
    pad = np.zeros((r, nw * 64), dtype=bool)
    pad[:, :n] = dense
    return np.packbits(pad, axis=-1, bitorder="little").reshape(r, nw * 8).view(np.int64).reshape(r, nw)


def oracle_stage2_arrays(exp, groups, n_points):
    ins = exp["ins"]
    nw = (n_points + 63) // 64
    offs, members = groups_arrays(groups)
    if len(exp["conf"]) == 0 and tuple(ins.shape) == (1, 0):                      # the reference's empty form
        return {"rows": np.zeros((0, nw), np.int64), "conf": exp["conf"].numpy(), "final_class": strings([]),
                "empty": np.asarray(True), "goffs": offs, "gmembers": members}
    assert ins.dtype == torch.bool and ins.shape[1] == n_points
    return {"rows": pack_bits(ins.numpy()), "conf": exp["conf"].numpy(), "final_class": strings(exp["final_class"]),
            "empty": np.asarray(False), "goffs": offs, "gmembers": members}


def oracle_final_arrays(exp):
    if isinstance(exp["ins"], list):
        assert exp["ins"] == [] and exp["conf"] == []
        return {"lists": np.asarray(True), "rows": np.zeros((0, 0), np.int64), "conf": np.zeros(0, np.float32),
                "final_class": strings(exp["final_class"])}
    return {"lists": np.asarray(False), "rows": pack_bits(exp["ins"].numpy()), "conf": exp["conf"].numpy(),
            "final_class": strings(exp["final_class"])}


def prefixed(prefix, arrays):
    return {f"{prefix}.{k}": v for k, v in arrays.items()}


def differences(got, exp, keys=None, skip=()):
    """Keys (of `exp`, or the given ones) whose arrays differ in dtype, shape or any element: [] when all agree.
    Numbers are compared with torch.equal, strings element by element."""
    bad = []
    for k in (sorted(exp) if keys is None else keys):
        if k.rsplit(".", 1)[-1] in skip:
            continue
        if k not in got or k not in exp:
            bad.append(k + " (missing)")
            continue
        a, b = np.asarray(got[k]), np.asarray(exp[k])
        if a.dtype.kind in "US" or b.dtype.kind in "US":
            same = a.shape == b.shape and a.tolist() == b.tolist()
        else:
            same = a.dtype == b.dtype and a.shape == b.shape and \
                torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))
        if not same:
            bad.append(k)
    return bad


# ------------------------------------------------------------------ one scene at a time: the references
def sequential_reference(case, names):
    """Every entry of `names` alone on the default stream, collected before the next starts, then the class with
    refinement.refine_class.  -> (arrays, the Stage2Results, the DeviceScenes)."""
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.refinement import refine_class
    devs = case.devices(names)
    out, results, trip = {}, [], []
    for j, name in enumerate(names):
        ds, st1 = devs[name]
        res = run_projection(ds, case.cfgs[name], stage1=st1)
        torch.cuda.synchronize()
        out.update(prefixed(f"s{j}", stage2_arrays(res, res.prefetch is not None)))
        results.append(res)
        trip.append((eid(j), st1, res))
    final = refine_class(trip, case.class_cfg(names), QUERY, case.sim(), DEV)
    torch.cuda.synchronize()
    for j in range(len(names)):
        out.update(prefixed(f"f{j}", final_arrays(final[eid(j)])))
    return out, results, devs


def sequential_finals(case, names, results_by_name):
    """The class of another list over Stage2Results already computed (their prefetch is used up: pass 1 decodes)."""
    from beyond_fixed_forms_amd.refinement import prepare_stage1, refine_class
    trip = [(eid(j), prepare_stage1(case.scenes[n].stage1, DEV), results_by_name[n]) for j, n in enumerate(names)]
    final = refine_class(trip, case.class_cfg(names), QUERY, case.sim(), DEV)
    torch.cuda.synchronize()
    out = {}
    for j in range(len(names)):
        out.update(prefixed(f"f{j}", final_arrays(final[eid(j)])))
    return out


def chunk_finals(case, names, results, size):
    """The list as classes of `size` consecutive entries (bench.py's --class-batch), each refined one at a time over the
    Stage2Results of sequential_reference."""
    from beyond_fixed_forms_amd.refinement import prepare_stage1, refine_class
    out = {}
    for at in range(0, len(names), size):
        js = range(at, min(at + size, len(names)))
        trip = [(eid(j), prepare_stage1(case.scenes[names[j]].stage1, DEV), results[j]) for j in js]
        final = refine_class(trip, case.class_cfg(names), QUERY, case.sim(), DEV)
        torch.cuda.synchronize()
        for j in js:
            out.update(prefixed(f"f{j}", final_arrays(final[eid(j)])))
    return out


def oracle_chunk_finals(case, names, per_scene, size):
    from oracle.refinement_ref import refine_class_ref
    out = {}
    for at in range(0, len(names), size):
        js = range(at, min(at + size, len(names)))
        trip = [(eid(j), case.scenes[names[j]].stage1,
                 {k: (v.clone() if torch.is_tensor(v) else list(v)) for k, v in per_scene[names[j]][0].items()}) for j in js]
        final = refine_class_ref(trip, case.class_cfg(names), QUERY, case.enc)
        for j in js:
            out.update(prefixed(f"f{j}", oracle_final_arrays(final[eid(j)])))
    return out


def oracle_scenes(case, names):
    """name -> (stage-2 dict, groups) of the oracle, once per distinct scene."""
    from oracle.projection_ref import project_scene_ref
    out = {}
    for name in dict.fromkeys(names):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            exp, dbg = project_scene_ref(case.oracle_scene(name), case.cfgs[name], return_debug=True)
        out[name] = (exp, dbg.get("groups", []))
    return out


def oracle_reference(case, names, per_scene):
    """Arrays of the oracle for the list: its stage 2 per entry and its refinement of the class."""
    from oracle.refinement_ref import refine_class_ref
    out, trip = {}, []
    for j, name in enumerate(names):
        exp, groups = per_scene[name]
        out.update(prefixed(f"s{j}", oracle_stage2_arrays(exp, groups, case.scenes[name].points.shape[0])))
        trip.append((eid(j), case.scenes[name].stage1,
                     {k: (v.clone() if torch.is_tensor(v) else list(v)) for k, v in exp.items()}))
    final = refine_class_ref(trip, case.class_cfg(names), QUERY, case.enc)
    for j in range(len(names)):
        out.update(prefixed(f"f{j}", oracle_final_arrays(final[eid(j)])))
    return out


# ------------------------------------------------------------------ timing: the scene call alone, the delay
def scene_call_ms(case, names):
    """Time on the device (events on the default stream, nothing else in flight) of the longest scene of the list, from
    the issue of its scene call to the end of its back half: the general and the step path do device work of their
    own there, and the host's few NumPy lines in between only lengthen what the delay is sized by.  Every scene is
    run once before it is timed, so that its workspace is sized and its tables remembered."""
    from beyond_fixed_forms_amd.projection import projection_back, projection_front
    devs = case.devices(names)
    worst = 0.0
    for name, (ds, st1) in devs.items():
        cfg = case.cfgs[name]
        projection_back(projection_front(ds, cfg, stage1=st1))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        projection_back(projection_front(ds, cfg, stage1=st1))
        e1.record()
        torch.cuda.synchronize()
        worst = max(worst, e0.elapsed_time(e1))
    return worst


def _sleep_ms(cycles):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(int(cycles))
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate_delay(scene_ms):
    """Cycles of torch.cuda._sleep that hold a stream for four times `scene_ms` and at least 20 ms (the host halves
    of the neighbours, a few tenths of a millisecond each, and the issue of a class's pass 2 must fit into it too),
    measured with events: -> (cycles, measured ms).  The delay is a condition of the skewed cases, so it is checked
    here: at least three scene calls long -- a held-back stream really finishes after its neighbours -- and at most
    DELAY_CAP_MS."""
    target = max(4.0 * scene_ms, 20.0)
    assert target <= 0.8 * DELAY_CAP_MS, f"scene call of {scene_ms:.3f} ms: the delay would exceed {DELAY_CAP_MS} ms"
    cycles = 1 << 17
    _sleep_ms(cycles)                                   # the first launch of the kernel
    ms = _sleep_ms(cycles)
    while ms < 0.5 and cycles < (1 << 34):              # a probe long enough to measure (under 4 ms)
        cycles *= 8
        ms = _sleep_ms(cycles)
    cycles = int(cycles * target / ms) + 1
    got = _sleep_ms(cycles)
    assert 3.0 * scene_ms <= got <= DELAY_CAP_MS, f"delay {got:.3f} ms for a scene call of {scene_ms:.3f} ms"
    return cycles, got


# ------------------------------------------------------------------ the runs
class Run:
    def __init__(self, arrays, devices, streams, seconds, busy=None):
        self.arrays, self.devices, self.streams, self.seconds = arrays, devices, streams, seconds
        self.busy = busy            # per class: (position of its last scene, per stream: still working after pass 2 was issued?)


def poison(batches, results):
    """A run's device results overwritten with ones before they are freed.  Runs repeat the same allocations, so
    torch's allocator hands the next run the blocks of this one: a kernel that read its input before the producer
    on another stream had written it would otherwise find the right values there, left by the run before."""
    for res in results:
        res.rows.fill_(-1)
    for batch in batches:
        for st in batch.refiner.states:
            for t in (st.matched1, st.stage2_rows, st.other1):
                if torch.is_tensor(t):
                    t.fill_(-1)
        for f in (batch.final or {}).values():
            if f.rows is not None:
                f.rows.fill_(-1)
    torch.cuda.synchronize()


def run_mixed(case, names, depth, reverse=False, before_front=None, before_add=None, class_size=None):
    """The list as bench.py's timed loop runs it: entry i on stream i % depth with that stream's workspace, `depth`
    scenes in flight, one class fed in the back halves and finished in the last one.  Entries keep the number j they
    have in `names` also when the list runs reversed.  before_front(i) / before_add(i) run on entry i's stream.
    class_size: classes of that many consecutive scenes, each finished in the back half of its last one."""
    from beyond_fixed_forms_amd import _lib, distributed as bdist
    from beyond_fixed_forms_amd.pipeline import pipelined, scene_streams
    from beyond_fixed_forms_amd.projection import projection_back, projection_front
    n = len(names)
    order = list(range(n))[::-1] if reverse else list(range(n))
    devs = case.devices(names)
    streams = scene_streams(DEV, depth)
    size = class_size or n
    batches, busy = [], []
    kept = {}
    t0 = time.perf_counter()

    def front(i):
        name = names[order[i]]
        ds, st1 = devs[name]
        with _lib.on_stream(streams[i % depth]):
            if before_front is not None:
                before_front(i)
            return projection_front(ds, case.cfgs[name], stage1=st1)

    def back(i, fr):
        j = order[i]
        with _lib.on_stream(streams[i % depth]):
            res = projection_back(fr)
            kept[j] = (res, res.prefetch is not None)
            if before_add is not None:
                before_add(i)
            if i % size == 0:
                ids = [eid(order[q]) for q in range(i, min(i + size, n))]
                batches.append(bdist.ClassBatch(case.class_cfg(names), QUERY, case.sim(), DEV, ids, len(ids)))
            batches[-1].add(eid(j), devs[names[j]][1], res)
            if (i + 1) % size == 0 or i + 1 == n:
                batches[-1].finish()
                busy.append((i, [not st.query() for st in streams]))

    for _ in pipelined(n, front, back, depth):
        pass
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    final = {sid: f for batch in batches for sid, f in batch.final.items()}
    out = {}
    for j in range(n):
        out.update(prefixed(f"s{j}", stage2_arrays(*kept[j])))
        out.update(prefixed(f"f{j}", final_arrays(final[eid(j)])))
    poison(batches, [res for res, _pre in kept.values()])
    return Run(out, devs, streams, seconds, busy)


def run_project_stream(case, names, depth, n_loaders, before_add=None, fail_at=None):
    """pipeline.project_stream over the list (loader threads, fresh DeviceScenes), the class fed in `consume` and
    finished afterwards as distributed.run_class does.  fail_at: `consume` raises KeyError at that scene."""
    from beyond_fixed_forms_amd import distributed as bdist
    from beyond_fixed_forms_amd.pipeline import project_stream, scene_streams
    n = len(names)
    batch = bdist.ClassBatch(case.class_cfg(names), QUERY, case.sim(), DEV, [eid(j) for j in range(n)], n)
    kept = {}
    t0 = time.perf_counter()

    def consume(k, st1, res):
        if k == fail_at:
            raise KeyError(k)
        kept[k] = (res, res.prefetch is not None)
        if before_add is not None:
            before_add(k)
        batch.add(eid(k), st1, res)

    project_stream([case.scenes[name] for name in names], case.cfgs[names[0]], DEV, consume, n_loaders=n_loaders,
                   depth=depth, want_groups=True)
    batch.finish()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    out = {}
    for j in range(n):
        out.update(prefixed(f"s{j}", stage2_arrays(*kept[j])))
        out.update(prefixed(f"f{j}", final_arrays(batch.final[eid(j)])))
    poison([batch], [res for res, _pre in kept.values()])
    return Run(out, None, scene_streams(DEV, depth), seconds)


def half_masks(scene):
    return scene.mask_2d[::2]


def class_items(case, names):
    """(SceneClasses, classes) per entry: the class "full" over every scene, "half" (every second mask frame) over
    the entries with an even number."""
    from beyond_fixed_forms_amd.scene import SceneClasses
    return [(SceneClasses(case.scenes[name], {"full": case.scenes[name].mask_2d, "half": half_masks(case.scenes[name])}),
             ["full", "half"] if j % 2 == 0 else ["full"]) for j, name in enumerate(names)]


def run_project_classes_stream(case, names, depth, n_loaders):
    """pipeline.project_classes_stream over class_items: arrays `s<j>.*` of class "full", `h<j>.*` of class "half"."""
    from beyond_fixed_forms_amd.pipeline import project_classes_stream, scene_streams
    items = class_items(case, names)
    kept, seen = {}, []
    t0 = time.perf_counter()

    def consume(k, cls, _st1, res):
        seen.append((k, cls))
        kept[(k, cls)] = res

    project_classes_stream(items, case.cfgs[names[0]], DEV, consume, n_loaders=n_loaders, depth=depth, want_groups=True)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    assert seen == [(k, c) for k, (_src, classes) in enumerate(items) for c in classes]
    out = {}
    for (k, cls), res in kept.items():
        out.update(prefixed(f"{'s' if cls == 'full' else 'h'}{k}", stage2_arrays(res, res.prefetch is not None)))
    return Run(out, None, scene_streams(DEV, depth), seconds)


def half_reference(case, names):
    """Class "half" of every even entry, alone on the default stream."""
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.scene import prepare_scene
    from beyond_fixed_forms_amd.synthetic import class_scene
    out, done = {}, {}
    for j, name in enumerate(names):
        if j % 2:
            continue
        if name not in done:
            sc = class_scene(case.scenes[name], half_masks(case.scenes[name]))
            res = run_projection(prepare_scene(sc, case.cfgs[name], device=DEV), case.cfgs[name])
            torch.cuda.synchronize()
            done[name] = stage2_arrays(res, False)
        out.update(prefixed(f"h{j}", done[name]))
    return out


def workspaces(streams):
    """The SceneWorkspace of each of `streams` (None for a stream that never ran a scene call)."""
    from beyond_fixed_forms_amd.pipeline import SceneWorkspace
    return [SceneWorkspace._per_stream.get((st.device.index, st.cuda_stream)) for st in streams]


def check_drained(streams):
    """After a run has been drained: no workspace is in flight, and a workspace that is not marked dirty has an
    all-zero row arena (as test_row_arena_recycling asserts for one stream).  -> number of workspaces looked at."""
    torch.cuda.synchronize()
    used = 0
    for k, ws in enumerate(workspaces(streams)):
        if ws is None:
            continue
        used += 1
        assert not ws.in_flight, f"workspace of stream {k} still in flight"
        if not ws.rows_dirty:
            assert int(ws.t["rows"].count_nonzero()) == 0, f"row arena of stream {k} is not zero"
    return used


def hold_stream(s, depth, cycles):
    """before_front hook: stream s is held back by the delay before each of its scene calls."""
    def hook(i):
        if i % depth == s:
            torch.cuda._sleep(cycles)
    return hook


def hold_every_second(cycles, which=0):
    """before_add hook: the delay on the stream of every second scene, before its pass 1 is enqueued.  Every small
    upload of a back half goes through _lib.upload's ring of eight pinned buffers, and the host waits for the copy
    that used a buffer eight uploads earlier: a pass 2 can only be issued ahead of a held-back pass 1 when fewer
    than eight uploads lie between the two, i.e. when the class ends with the scene after the held-back one."""
    def hook(i):
        if i % 2 == which:
            torch.cuda._sleep(cycles)
    return hook


# ------------------------------------------------------------------ the child of the stream-switch test
def worker(out_path, scenes_file=None):
    """The depth-4 pass over MIXED and the same pass with stream 1 held back, in a process of its own (the two
    switches as inherited) -> one .npz of everything delivered, the streams the workspaces carry, and the times."""
    t0 = time.perf_counter()
    from beyond_fixed_forms_amd import _lib, pipeline
    _lib.load()
    case = Case(scenes_file)
    depth = pipeline.PIPELINE_DEPTH
    plain = run_mixed(case, MIXED, depth)
    used = check_drained(plain.streams)
    scene_ms = scene_call_ms(case, MIXED)
    cycles, delay_ms = calibrate_delay(scene_ms)
    skew = run_mixed(case, MIXED, depth, before_front=hold_stream(1, depth, cycles))
    check_drained(skew.streams)
    out = {}
    out.update(prefixed("plain", plain.arrays))
    out.update(prefixed("skew", skew.arrays))
    wss = [ws for ws in workspaces(plain.streams) if ws is not None]
    heavy = [int(ws.struct.heavy_stream or 0) for ws in wss]
    aux = [int(ws.struct.aux_stream or 0) for ws in wss]
    out["meta.workspaces"] = np.asarray(used)
    out["meta.heavy_handles"] = np.asarray(heavy, dtype=np.uint64)
    out["meta.aux_handles"] = np.asarray(aux, dtype=np.uint64)
    out["meta.heavy_events"] = np.asarray([sum(1 for e in ws.struct.events if e) for ws in wss])
    out["meta.aux_events"] = np.asarray([sum(1 for e in ws.struct.aux_events if e) for ws in wss])
    out["meta.switches"] = np.asarray([pipeline.HEAVY_STREAMS, int(pipeline.AUX_STREAM)])
    out["meta.scene_ms"] = np.asarray(scene_ms)
    out["meta.delay_ms"] = np.asarray(delay_ms)
    out["meta.seconds"] = np.asarray(time.perf_counter() - t0)
    np.savez(out_path, **out)
    print(f"pipelined child: heavy {pipeline.HEAVY_STREAMS} aux {int(pipeline.AUX_STREAM)}: longest scene {scene_ms:.3f} ms, "
          f"delay {delay_ms:.3f} ms, {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    worker(*sys.argv[1:3])
