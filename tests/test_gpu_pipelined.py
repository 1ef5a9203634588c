"""Scenes in flight on several streams against one-at-a-time runs.

Every published number comes from PIPELINE_DEPTH scenes in flight, each on its own stream with its own SceneWorkspace,
loader threads uploading on further streams, the host half of scene i under the kernels of its neighbours and a class's
pass 2 on whichever stream came last.  What keeps that correct has no kernel to compare -- waits on events, the
workspaces' in_flight / rows_dirty flags, the re-issues inside pipeline.collect, `both` outliving its workspace -- so
here one list of small scenes that takes every path of the scene call (pipelined_case.MIXED) runs pipelined and must
deliver, array for array, what each scene delivers alone on the default stream, which in turn equals the oracle:

 1. as bench.py's loop at depth 1, 2 and 4, in list order and reversed; with every scene re-issued for the sorting
    filter; through project_stream / project_classes_stream with 1 and 2 loaders; after an abandoned project_stream;
 2. the depth-4 runs again with one stream held back by a device-side delay of several scene calls (a scene stream
    before its call, the streams of every second scene before pass 1 with classes of two scenes, the loaders' streams
    before the uploads);
 3. in fresh child processes under BFF_HEAVY_STREAMS / BFF_AUX_STREAM, which move parts of the scene call to further
    streams behind event hand-overs."""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pipelined_case as pc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = pc.DEV
ROOT = pc.ROOT


@pytest.fixture(scope="module")
def case():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return pc.Case()


@pytest.fixture(scope="module")
def depth():
    from beyond_fixed_forms_amd.pipeline import PIPELINE_DEPTH
    assert len(pc.MIXED) >= 2 * PIPELINE_DEPTH + 2
    return PIPELINE_DEPTH


class Reference:
    pass


@pytest.fixture(scope="module")
def ref(case):
    """Once per module, nothing else in flight: every entry of MIXED alone on the default stream + refine_class, the
    oracle for the same list, and both again for the same-sized list project_stream takes."""
    r = Reference()
    r.mixed, results, devs = pc.sequential_reference(case, pc.MIXED)
    r.group_cap = {name: ds.__dict__.get("_group_cap") for name, (ds, _st1) in devs.items()}
    per_scene = pc.oracle_scenes(case, pc.MIXED)
    r.groups = {name: len(g) for name, (_exp, g) in per_scene.items()}
    r.oracle_mixed = pc.oracle_reference(case, pc.MIXED, per_scene)
    # the same-sized list: stage 2 of an entry is that of the same scene in MIXED, the class is another one
    first = {name: pc.MIXED.index(name) for name in pc.SAME_SIZED}
    r.same = {}
    for j, name in enumerate(pc.SAME_SIZED):
        r.same.update({f"s{j}.{k.split('.', 1)[1]}": v for k, v in r.mixed.items() if k.startswith(f"s{first[name]}.")})
    r.same.update(pc.sequential_finals(case, pc.SAME_SIZED, {name: results[j] for name, j in first.items()}))
    r.oracle_same = pc.oracle_reference(case, pc.SAME_SIZED, per_scene)
    r.half = pc.half_reference(case, pc.SAME_SIZED)
    # MIXED as classes of two consecutive scenes (the same pairs when the list runs reversed)
    assert len(pc.MIXED) % 2 == 0
    r.pairs = pc.chunk_finals(case, pc.MIXED, results, 2)
    r.oracle_pairs = pc.oracle_chunk_finals(case, pc.MIXED, per_scene, 2)
    torch.cuda.synchronize()
    return r


@pytest.fixture(scope="module")
def delay(case, ref):
    """The device-side delay of the skewed cases, calibrated, not hard-coded: torch.cuda._sleep cycles for four times
    the device time of the longest scene of the list run alone and at least 20 ms (pipelined_case.calibrate_delay
    asserts that the measured delay is at least three such scenes and at most 100 ms)."""
    scene_ms = pc.scene_call_ms(case, pc.MIXED)
    cycles, delay_ms = pc.calibrate_delay(scene_ms)
    print(f"\nlongest scene alone {scene_ms:.3f} ms, calibrated delay {delay_ms:.3f} ms ({cycles} cycles)")
    assert 3.0 * scene_ms <= delay_ms <= pc.DELAY_CAP_MS
    return cycles


def keys_of(arrays, prefixes, leaves=None):
    return [k for k in sorted(arrays) if k.split(".")[0][0] in prefixes and (leaves is None or k.split(".")[1] in leaves)]


def check_mixed(run, ref):
    """A pipelined run of MIXED: every Stage2Result and FinalResult equals the one-at-a-time reference and the oracle,
    the group capacity was remembered, the workspaces are drained."""
    assert pc.differences(run.arrays, ref.mixed) == []
    assert pc.differences(run.arrays, ref.oracle_mixed) == []
    assert run.devices["g325"][0].__dict__.get("_group_cap") == 512
    assert pc.check_drained(run.streams) == len(run.streams)


# ------------------------------------------------------------------ 0. the conditions
def test_reference_takes_every_path_and_equals_the_oracle(ref):
    """What the other tests presuppose: alone on the default stream each scene takes the path it is in the list for, the
    325-group scene remembers the large tables after its first visit, the class has final instances, and the
    one-at-a-time results equal the oracle's (stage 2, groups and final results)."""
    for j, name in enumerate(pc.MIXED):
        assert str(ref.mixed[f"s{j}.path"]) == pc.SCENES[name][2], name
        if pc.SCENES[name][2] == "fast" and ref.mixed[f"s{j}.rows"].shape[0]:
            assert bool(ref.mixed[f"s{j}.prefetch"]), name
    assert 256 < ref.groups["g325"] <= 512 < ref.groups["g552"]
    assert ref.group_cap["g325"] == 512
    assert ref.mixed["s1.rows"].shape[1] * 64 != 4001 and ref.mixed["s2.rows"].shape[1] > ref.mixed["s0.rows"].shape[1]
    assert bool(ref.mixed["s5.empty"]) and ref.mixed["s5.rows"].shape[0] == 0
    for arrays in (ref.mixed, ref.same):
        n = len([k for k in arrays if k.endswith(".lists")])
        assert sum(arrays[f"f{j}.rows"].shape[0] for j in range(n)) >= 1
        assert all(not bool(arrays[f"f{j}.lists"]) for j in range(n))
    assert pc.differences(ref.mixed, ref.oracle_mixed) == []
    assert pc.differences(ref.same, ref.oracle_same) == []
    assert pc.differences(ref.pairs, ref.oracle_pairs) == []


# ------------------------------------------------------------------ 1. in flight, friendly timing
@pytest.mark.parametrize("reverse", [False, True], ids=["list_order", "reversed"])
@pytest.mark.parametrize("d", [1, 2, 4])
def test_mixed_scenes_in_flight(case, ref, depth, d, reverse):
    """The list as bench.py runs it, fresh DeviceScenes, `d` scenes in flight: with four streams every workspace is
    reused twice with another shape while its neighbours run."""
    assert d <= depth
    check_mixed(pc.run_mixed(case, pc.MIXED, d, reverse=reverse), ref)


def test_every_scene_reissued_under_load(case, ref, depth):
    """The value set of the point filter shrunk to one value for a whole pass: every scene call overflows and is issued
    again with the sorting formulation inside pipeline.collect while three other scenes run (the 325-group scene a third
    time for its tables).  Same results, and every scene remembers the sorting formulation."""
    from beyond_fixed_forms_amd import _lib
    lib = _lib.load()
    assert lib.bff_point_threshold_capacity_set(1) == 1
    try:
        run = pc.run_mixed(case, pc.MIXED, depth)
    finally:
        lib.bff_point_threshold_capacity_set(0)
    check_mixed(run, ref)
    for name, (ds, _st1) in run.devices.items():
        if pc.SCENES[name][2] != "step":
            assert ds.__dict__.get("_filter_sort") is True, name


@pytest.mark.parametrize("n_loaders", [1, 2])
@pytest.mark.parametrize("d", [1, 2, 4])
def test_project_stream_and_project_classes_stream(case, ref, d, n_loaders):
    """Both streaming entry points over the same-sized list, which holds the two group-capacity cases (their DeviceScenes
    are new every time, so the 325-group scene is re-issued twice per run under load): project_stream with the class
    fed in `consume`; project_classes_stream with two classes per scene, "half" over the even entries only.  Each
    (scene, class) equals its sequential reference."""
    run = pc.run_project_stream(case, pc.SAME_SIZED, d, n_loaders)
    assert pc.differences(run.arrays, ref.same) == []
    assert pc.differences(run.arrays, ref.oracle_same) == []
    assert pc.check_drained(run.streams) == d
    runc = pc.run_project_classes_stream(case, pc.SAME_SIZED, d, n_loaders)
    n = len(pc.SAME_SIZED)
    assert sorted(runc.arrays) == sorted(keys_of(ref.same, "s") + list(ref.half))
    assert len(ref.half) == 8 * ((n + 1) // 2)
    assert pc.differences(runc.arrays, ref.same, keys=keys_of(ref.same, "s"), skip=("prefetch",)) == []   # no stage 1 here
    assert pc.differences(runc.arrays, ref.half) == []
    assert pc.check_drained(runc.streams) == d


def test_abandoned_project_stream(case, ref, depth):
    """`consume` raises at scene 2 of project_stream: the exception surfaces, the loader threads are gone, three fronts
    were issued and never collected.  A second project_stream over the same streams gives the reference results:
    nothing of the abandoned calls leaks into it."""
    from beyond_fixed_forms_amd.pipeline import scene_streams
    with pytest.raises(KeyError):
        pc.run_project_stream(case, pc.SAME_SIZED, depth, 2, fail_at=2)
    assert not [t for t in threading.enumerate() if t.name.startswith("bff-loader")]
    abandoned = [ws for ws in pc.workspaces(scene_streams(DEV, depth)) if ws is not None and ws.in_flight]
    assert len(abandoned) >= 2                       # issued, never collected (one of the three is the step path)
    run = pc.run_project_stream(case, pc.SAME_SIZED, depth, 2)
    assert pc.differences(run.arrays, ref.same) == []
    assert pc.check_drained(run.streams) == depth
    assert not [t for t in threading.enumerate() if t.name.startswith("bff-loader")]


# ------------------------------------------------------------------ 2. skewed timing
@pytest.mark.parametrize("reverse", [False, True], ids=["list_order", "reversed"])
@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_one_scene_stream_held_back(case, ref, depth, delay, s, reverse):
    """(a) the delay on scene stream s before each of its scene calls: its scenes finish after their neighbours', the
    host collects in order all the same, and the class's pass 2 reads their rows from another stream."""
    assert s < depth
    check_mixed(pc.run_mixed(case, pc.MIXED, depth, reverse=reverse, before_front=pc.hold_stream(s, depth, delay)), ref)


@pytest.mark.parametrize("reverse", [False, True], ids=["list_order", "reversed"])
def test_pass_one_of_every_second_scene_held_back(case, ref, depth, delay, reverse):
    """(b) the delay in the back half of every second scene, on its stream, before the class takes it, with classes of
    two scenes as bench.py's --class-batch forms them: the class is finished in the back half of the next scene, on that
    scene's stream, and its pass 2 must wait for the held-back scene's `ready` event.  (With one class over the whole
    list the host never gets ahead of a held-back stream: pipelined_case.hold_every_second.)  As conditions: after pass
    2 of a class had been issued the held-back stream was still working -- no host wait sat the delay out -- and such
    a scene has final instances, so a pass 2 that ran ahead would show."""
    n = len(pc.MIXED)
    run = pc.run_mixed(case, pc.MIXED, depth, reverse=reverse, before_add=pc.hold_every_second(delay, 0), class_size=2)
    late = [i - 1 for i, busy in run.busy if busy[(i - 1) % depth]]          # held-back positions still at work
    print(f"\nheld-back scenes still at work after their class's pass 2 was issued: positions {late} of {n // 2}")
    assert len(run.busy) == n // 2 and late
    assert sum(ref.pairs[f"f{(n - 1 - i) if reverse else i}.rows"].shape[0] for i in late) >= 1
    finals = keys_of(ref.pairs, "f")
    assert pc.differences(run.arrays, ref.mixed, keys=keys_of(ref.mixed, "s")) == []
    assert pc.differences(run.arrays, ref.pairs, keys=finals) == []
    assert pc.differences(run.arrays, ref.oracle_pairs, keys=finals) == []
    assert pc.check_drained(run.streams) == depth


def test_loader_streams_held_back(case, ref, depth, delay, monkeypatch):
    """(c) the delay on the loader's stream before the uploads of every scene: the scene streams must wait for the
    loaders' events before they read what was uploaded (project_stream and project_classes_stream).  As a condition:
    scene calls were issued while the uploads of their scene were still held back on the loader's stream."""
    from beyond_fixed_forms_amd import ingest, projection
    calls, uploaded, early = [], {}, []

    def held(fn):
        def wrapped(*a, **kw):
            calls.append(fn.__name__)
            torch.cuda._sleep(delay)                 # on the current stream: the loader's
            out = fn(*a, **kw)
            ev = torch.cuda.Event()
            ev.record()                              # the loader's stream has come this far once the uploads are done
            uploaded[id(out)] = (out, ev)
            return out
        return wrapped

    front = projection.projection_front

    def watched_front(ds, *a, **kw):
        ev = uploaded.get(id(ds), (None, None))[1]
        early.append(ev is not None and not ev.query())
        return front(ds, *a, **kw)

    monkeypatch.setattr(ingest, "prepare_scene_fast", held(ingest.prepare_scene_fast))
    monkeypatch.setattr(ingest, "prepare_geometry_fast", held(ingest.prepare_geometry_fast))
    # the geometry's viewed counts make the loader thread wait for its stream, which sits the first delay out: the
    # classes' own tables are held back as well, so that their scene calls too can come before their uploads
    monkeypatch.setattr(ingest, "prepare_class_fast", held(ingest.prepare_class_fast))
    monkeypatch.setattr(projection, "projection_front", watched_front)
    run = pc.run_project_stream(case, pc.SAME_SIZED, depth, 2)
    assert calls.count("prepare_scene_fast") == len(pc.SAME_SIZED)
    print(f"\nproject_stream: {sum(early)} of {len(early)} scene calls issued before their uploads had finished")
    assert len(early) == len(pc.SAME_SIZED) and sum(early) >= 1
    assert pc.differences(run.arrays, ref.same) == []
    assert pc.check_drained(run.streams) == depth
    del early[:]
    runc = pc.run_project_classes_stream(case, pc.SAME_SIZED, depth, 2)
    assert calls.count("prepare_geometry_fast") == len(pc.SAME_SIZED)
    print(f"project_classes_stream: {sum(early)} of {len(early)} scene calls issued before their uploads had finished")
    assert sum(early) >= 1
    assert pc.differences(runc.arrays, ref.same, keys=keys_of(ref.same, "s"), skip=("prefetch",)) == []
    assert pc.differences(runc.arrays, ref.half) == []
    assert pc.check_drained(runc.streams) == depth


# ------------------------------------------------------------------ 3. the stream switches, one child each
# A child imports torch, loads the library, reads the saved scenes and runs two passes of ten tiny scenes: 10-20 s, most
# of it start-up.  The limit leaves that several times over for a busy machine and still ends a child that hangs.
CHILD_TIMEOUT_S = 120
SWITCHES = {
    "default": {},
    "heavy1": {"BFF_HEAVY_STREAMS": "1"},
    "heavy3": {"BFF_HEAVY_STREAMS": "3"},             # four workspaces share three heavy streams unevenly
    "aux": {"BFF_AUX_STREAM": "1"},
    "heavy2_aux": {"BFF_HEAVY_STREAMS": "2", "BFF_AUX_STREAM": "1"},
}


@pytest.fixture(scope="module")
def scenes_file(case, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("pipelined") / "scenes.pt")
    case.save_scenes(path)
    return path


stopped = []                 # a child that hung or crashed: no further child is started on that GPU


def run_child(name, scenes_file, out_dir):
    if stopped:
        pytest.fail(f"no child started: {stopped[0]}")
    env = {k: v for k, v in os.environ.items() if k not in ("BFF_HEAVY_STREAMS", "BFF_AUX_STREAM")}
    env.update(SWITCHES[name])
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = os.path.join(str(out_dir), f"{name}.npz")
    t0 = time.perf_counter()
    try:
        subprocess.run([sys.executable, os.path.abspath(pc.__file__), out, scenes_file], check=True, env=env, cwd=ROOT,
                       timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        stopped.append(f"the child {name} hung ({CHILD_TIMEOUT_S} s)")
        raise
    except subprocess.CalledProcessError as e:
        if e.returncode < 0 or e.returncode in (124, 134, 137, 139):        # killed by a signal, aborted, faulted
            stopped.append(f"the child {name} ended with status {e.returncode}")
        raise
    print(f"\nchild {name}: {time.perf_counter() - t0:.1f} s")
    return np.load(out)


@pytest.fixture(scope="module")
def default_child(scenes_file, tmp_path_factory):
    return run_child("default", scenes_file, tmp_path_factory.mktemp("pipelined_default"))


@pytest.mark.parametrize("name", list(SWITCHES))
def test_stream_switches(ref, depth, scenes_file, default_child, tmp_path, name):
    """The depth-4 pass and the pass with stream 1 held back under each value of the two switches: every array equals
    the default child's, the default child's equal the in-process reference, and the child's workspaces really carry
    the streams (and events) the switch asks for."""
    got = default_child if name == "default" else run_child(name, scenes_file, tmp_path)
    heavy = int(SWITCHES[name].get("BFF_HEAVY_STREAMS", "0"))
    aux = SWITCHES[name].get("BFF_AUX_STREAM") == "1"
    assert got["meta.switches"].tolist() == [heavy, int(aux)]
    assert int(got["meta.workspaces"]) == depth
    hh, ah = got["meta.heavy_handles"].tolist(), got["meta.aux_handles"].tolist()
    assert len(hh) == len(ah) == depth
    if heavy:
        assert all(hh) and len(set(hh)) == min(heavy, depth) and got["meta.heavy_events"].tolist() == [4] * depth
    else:
        assert not any(hh) and got["meta.heavy_events"].tolist() == [0] * depth
    if aux:
        assert all(ah) and len(set(ah)) == depth and got["meta.aux_events"].tolist() == [2] * depth
    else:
        assert not any(ah) and got["meta.aux_events"].tolist() == [0] * depth
    assert 3.0 * float(got["meta.scene_ms"]) <= float(got["meta.delay_ms"]) <= pc.DELAY_CAP_MS
    data = [k for k in got.files if not k.startswith("meta.")]
    assert sorted(data) == sorted(k for k in default_child.files if not k.startswith("meta."))
    assert len(data) == 2 * len(ref.mixed)
    assert pc.differences(got, default_child, keys=data) == []
    if name == "default":
        for part in ("plain", "skew"):
            assert pc.differences({k[len(part) + 1:]: got[k] for k in data if k.startswith(part + ".")}, ref.mixed) == []
