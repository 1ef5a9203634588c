"""The float64 references of tests/similarity_ref.py against the reference's own tensor expressions evaluated by torch on
the CPU in float64, the case table against the restated dispatch rule, and that rule against the library's host-only
bff_cosine_gemm_path (which launches nothing, so it answers without a GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import similarity_ref as sr


def special_inputs(na, nb, dim, seed):
    a, b = sr.randn_halves(na, nb, dim, seed)
    a[na // 2] = 0                                            # a zero row in each operand
    b[nb // 2] = 0
    return a, b


@pytest.mark.parametrize("na,nb,dim", [(1, 1, 32), (5, 7, 64), (16, 33, 96)])
def test_cosine_reference_is_the_tensor_expression(na, nb, dim):
    """R:109-114:  similarity = t1 @ t2.T;  similarity / (t1.norm(dim=-1, keepdim=True) * t2.norm(dim=-1, keepdim=True).T)."""
    for a, b in (sr.randn_halves(na, nb, dim), sr.integer_halves(na, nb, dim), special_inputs(na + 2, nb + 2, dim, 3)):
        t1, t2 = torch.from_numpy(a).double(), torch.from_numpy(b).double()
        similarity = t1 @ t2.T
        similarity = similarity / (t1.norm(dim=-1, keepdim=True) * t2.norm(dim=-1, keepdim=True).T)
        got = sr.cosine_ref(a, b)
        assert np.array_equal(np.isnan(got), torch.isnan(similarity).numpy())
        assert np.allclose(got, similarity.numpy(), rtol=0, atol=1e-14, equal_nan=True)
    got = sr.cosine_ref(*special_inputs(6, 5, 32, 4))
    assert np.isnan(got[3]).all() and np.isnan(got[:, 2]).all() and np.isfinite(np.delete(np.delete(got, 3, 0), 2, 1)).all()


@pytest.mark.parametrize("na,nb,dim", [(1, 1, 32), (5, 7, 64), (16, 33, 96)])
def test_normalised_reference_is_the_tensor_expression(na, nb, dim):
    """SEG:388-393:  F.normalize(region_embedding) @ capt_feature_ensembled.T  -- a zero box embedding is a row of 0.0."""
    for a, b in (sr.randn_halves(na, nb, dim), special_inputs(na + 2, nb + 2, dim, 5)):
        b = sr.spread_bank(b) if b.any(axis=1).all() else b
        exp = F.normalize(torch.from_numpy(a).double()) @ torch.from_numpy(b).double().T
        got = sr.normalized_ref(a, b)
        assert np.isfinite(got).all() and np.allclose(got, exp.numpy(), rtol=0, atol=1e-14)
    got = sr.normalized_ref(*special_inputs(6, 5, 32, 4))
    assert (got[3] == 0).all() and (got[:, 2] == 0).all() and (np.delete(np.delete(got, 3, 0), 2, 1) != 0).all()


def test_spread_bank_spans_the_norms_and_separates_the_two_forms():
    """Norms over 0.25 .. 4, and at every shape of the table the normalised product is far (> 10 bounds) from the cosine
    somewhere: a kernel that normalised the columns anyway cannot pass."""
    for na, nb, dim, _ in sr.CASES:
        if na * nb * dim > 2_000_000:
            na = 64                                           # the property is the bank's: fewer rows of A show it as well
        a, b = sr.randn_halves(na, nb, dim)
        b = sr.spread_bank(b)
        norms = np.linalg.norm(b.astype(np.float64), axis=1)
        assert 0.24 <= norms.min() and norms.max() <= 4.1
        if nb >= 8:
            assert norms.min() < 0.3 and norms.max() > 3.5
        assert np.abs(sr.normalized_ref(a, b) - sr.cosine_ref(a, b)).max() > 10 * 1e-4 * norms.max(), (na, nb, dim)


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 768])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_description_means_reference_is_the_tensor_expression(dim, dtype):
    """SEG:324-337:  F.normalize(encodings) per class;  cat([x.mean(dim=0).reshape(1, -1)]);  /= norm(dim=-1, keepdim=True)."""
    desc, offs = sr.description_inputs(dim, dtype)
    classes = [torch.from_numpy(desc[offs[c]:offs[c + 1]]).double() for c in range(len(offs) - 1)]
    encodings = [F.normalize(x) for x in classes]
    descr_means = torch.cat([x.mean(dim=0).reshape(1, -1) for x in encodings])
    descr_means /= descr_means.norm(dim=-1, keepdim=True)
    got = sr.description_means_ref(desc, offs)
    assert np.isnan(got[2]).all() and np.isfinite(np.delete(got, 2, 0)).all()
    assert np.allclose(got, descr_means.numpy(), rtol=0, atol=1e-14, equal_nan=True)


def test_description_inputs_are_not_degenerate():
    for dim in (1, 63, 64, 65, 768, 2048):
        for dtype in (np.float32, np.float16):
            desc, offs = sr.description_inputs(dim, dtype)
            unit = sr.normalize_ref(desc)
            for c in (0, 1, 3):
                assert np.linalg.norm(unit[offs[c]:offs[c + 1]].mean(0)) > 0.2
            assert not desc[6].any() and np.abs(desc[[5, 7]]).sum(1).min() > 0 and offs[3] <= 5 and offs[4] > 7


# ------------------------------------------------------------------ the case table and the dispatch rule
def test_case_table_covers_every_path_twice():
    by_path = {p: 0 for p in range(6)}
    for na, nb, dim, path in sr.CASES:
        assert sr.gemm_path(na, nb, dim) == path, (na, nb, dim)
        by_path[path] += 1
    for variant in sr.VARIANTS:
        for shape in sr.VARIANT_SHAPES:
            by_path[sr.variant_path(variant, *shape)] += variant != "default"
    assert all(n >= 2 for n in by_path.values()), by_path
    assert len(set(sr.CASES)) == len(sr.CASES)
    assert max(na * dim for na, _, dim, _ in sr.CASES) == 16400 * 768          # the largest operand
    assert [sr.variant_path(v, 2063, 200, 768) for v in sr.VARIANTS] == [3, 2, 4]
    assert [sr.variant_path(v, 4100, 198, 512) for v in sr.VARIANTS] == [5, 2, 5]
    assert set(sr.VARIANT_SHAPES) <= {c[:3] for c in sr.CASES}
    assert [c[3] for c in sr.SPECIAL_SHAPES] == [0, 1, 2, 3, 5] and set(sr.SPECIAL_SHAPES) <= set(sr.CASES)


def test_integer_inputs_are_exact_in_float32():
    for na, nb, dim in [(1, 1, 32), (40, 3, 2048), (17, 209, 160)]:
        a, b = sr.integer_halves(na, nb, dim)
        for m in (a, b):
            assert np.array_equal(m, np.round(m)) and np.abs(m).max() <= 31 and m.any(axis=1).all()
        assert sorted(np.unique(a)) != sorted(np.unique(b))                    # drawn differently
        bits, raw = sr.exact_bits(a, b)                                         # asserts the 2^24 bounds itself
        assert bits.dtype == np.float32 and np.abs(bits.astype(np.float64) - sr.cosine_ref(a, b)).max() < 2e-7
        assert raw.dtype == np.float32 and np.allclose(raw, sr.normalized_ref(a, b), rtol=3e-7, atol=0)
    # no all-zero row survives the redraw
    a, _ = sr.integer_halves(4096, 1, 32, seed=7)
    assert a.any(axis=1).all()


def boundary_shapes():
    shapes = [c[:3] for c in sr.CASES]
    for na in (0, 1, 2047, 2048):
        for nb in (0, 1, 64, 65, 256, 257):
            for dim in (0, 31, 32, 512, 736, 768, 1024):
                shapes.append((na, nb, dim))
    return shapes + [(-1, 5, 32), (5, -1, 32), (5, 5, -32)]


def library():
    from beyond_fixed_forms_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    return _lib


def test_rule_equals_the_library_in_this_process():
    _lib = library()
    bank = os.environ.get("BFF_GEMM_BANK")
    stage = os.environ.get("BFF_GEMM_STAGE")
    kw = dict(bank=bank is None or int(bank) != 0, stage=2 if stage is None else int(stage))
    for shape in boundary_shapes():
        assert _lib.cosine_gemm_path(*shape) == sr.gemm_path(*shape, **kw), shape
    assert len(_lib.GEMM_PATHS) == 6 == len(sr.PATH_NAMES)


CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
print(json.dumps([lib.bff_cosine_gemm_path(*s) for s in json.loads(sys.argv[2])]))
"""


@pytest.mark.parametrize("variant", list(sr.VARIANTS))
def test_rule_equals_the_library_under_each_switch(variant):
    """The switches are read once per process: each value gets a fresh child, which only loads the library and asks."""
    import json
    _lib = library()
    shapes = boundary_shapes()
    env = {k: v for k, v in os.environ.items() if k not in ("BFF_GEMM_BANK", "BFF_GEMM_STAGE")}
    env.update(sr.VARIANTS[variant])
    out = subprocess.run([sys.executable, "-c", CHILD, _lib.LIB_PATH, json.dumps(shapes)], check=True, env=env,
                         capture_output=True, text=True, timeout=120).stdout
    got = json.loads(out.strip().splitlines()[-1])
    assert got == [sr.variant_path(variant, *s) for s in shapes]
    assert {3: "default", 2: "bank0", 4: "stage4"}[got[shapes.index((2063, 200, 768))]] == variant


def test_gemm_wrappers_refuse_unequal_widths_before_any_call(monkeypatch):
    """512-d box features against a 768-d bank: refused by the wrapper itself (the C entry point takes one `dim`)."""
    _lib = library()
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("the library was called with unequal widths"))
    monkeypatch.setattr(_lib, "_ptr", lambda *a, **k: None)               # host tensors stand in for device ones
    a, b = torch.zeros(4, 512, dtype=torch.float16), torch.zeros(3, 768, dtype=torch.float16)
    for fn in (_lib.cosine_gemm_f16, _lib.normalized_gemm_f16):
        with pytest.raises(ValueError, match="widths differ"):
            fn(a, b)
        with pytest.raises(ValueError, match="widths differ"):
            fn(b, a)
