"""csrc/cosine.hip on the device: the four matrix-core GEMM kernels (six instantiations) on every path of the dispatcher,
each path proved taken (bff_cosine_gemm_path), against the float64 statements of tests/similarity_ref.py and -- where the
arithmetic is exact -- bit for bit; bff_cosine_rows and bff_description_means at the sizes their guards exist for.

Run as a script (`python tests/test_gpu_similarity.py OUT.npz`) this file is the variant test's worker: BFF_GEMM_BANK and
BFF_GEMM_STAGE are read once per process, so each value gets a fresh child."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import similarity_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-4                                                    # BASELINE.json north_star: cosines to 1e-4 absolute
SENTINEL = 0x5EA7F00D                                         # as float32 2.4e18: no cosine, no product of these inputs


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def both(lib, a, b):
    """(cosine form, normalised form) of host arrays as float32 host arrays."""
    ta, tb = dev(a), dev(b)
    return host(lib.cosine_gemm_f16(ta, tb)), host(lib.normalized_gemm_f16(ta, tb))


def err(got, exp):
    return float(np.abs(got.astype(np.float64) - exp).max())


def case_id(c):
    return f"{sr.PATH_NAMES[c[3]]}-{c[0]}x{c[1]}x{c[2]}"


# ------------------------------------------------------------------ every path, proved taken
@pytest.mark.parametrize("case", sr.CASES, ids=case_id)
def test_gemm_paths(lib, case):
    na, nb, dim, path = case
    assert lib.cosine_gemm_path(na, nb, dim) == path
    rng = np.random.default_rng(na + nb + dim)

    # 1. random halves; the normalised form against a bank whose norms span 0.25 .. 4
    a, b = sr.randn_halves(na, nb, dim)
    ref = sr.cosine_ref(a, b)
    cos, _ = both(lib, a, b)
    e = err(cos, ref)
    print(f"randn cosine: {e:.3g}")
    assert cos.shape == (na, nb) and e <= BAR
    bs = sr.spread_bank(b)
    bmax = float(np.linalg.norm(bs.astype(np.float64), axis=1).max())
    cos_s, raw = both(lib, a, bs)
    e, apart = err(raw, sr.normalized_ref(a, bs)), err(raw, sr.cosine_ref(a, bs))
    print(f"randn normalised: {e:.3g} (bound {BAR * bmax:.3g}), from the cosine: {apart:.3g}")
    assert e <= BAR * bmax
    assert apart > BAR * bmax                                 # the columns were NOT normalised

    # 2. exact integers, bit for bit
    ai, bi = sr.integer_halves(na, nb, dim)
    cos_i, raw_i = both(lib, ai, bi)
    for name, got, exp in zip(("cosine", "normalised"), (cos_i, raw_i), sr.exact_bits(ai, bi)):
        diff = bits(got) != bits(exp)
        print(f"integers {name}: {int(diff.sum())} of {diff.size} differ")
        assert not diff.any(), (name, np.argwhere(diff)[:5], got[diff][:5], exp[diff][:5])

    # 3. scale invariance of the cosine form, bit for bit: A * 2^k is exact in float16 and in every float32 operation
    for k in (1, 6, 12):
        scaled = (a.astype(np.float32) * np.float32(2.0 ** k)).astype(np.float16)
        assert np.isfinite(scaled).all() and np.array_equal(scaled.astype(np.float64), a.astype(np.float64) * 2.0 ** k)
        got = host(lib.cosine_gemm_f16(dev(scaled), dev(b)))
        assert np.array_equal(bits(got), bits(cos)), (k, int((bits(got) != bits(cos)).sum()))

    # 4. permutations of the rows of A and of B: the same bits at the permuted places
    pa, pb = rng.permutation(na), rng.permutation(nb)
    cos_pa, raw_pa = both(lib, a[pa], bs)
    assert np.array_equal(bits(cos_pa), bits(cos_s[pa])) and np.array_equal(bits(raw_pa), bits(raw[pa]))
    cos_pb, raw_pb = both(lib, a, bs[pb])
    assert np.array_equal(bits(cos_pb), bits(cos_s[:, pb])) and np.array_equal(bits(raw_pb), bits(raw[:, pb]))

    # 5. the magnitude of normalised CLIP features: a few entries per row are float16 subnormals
    small = (a.astype(np.float32) / np.float32(32)).astype(np.float16)
    small_b = (b.astype(np.float32) / np.float32(32)).astype(np.float16)
    if na * dim >= 100_000:
        assert (np.abs(small[small != 0]) < 2.0 ** -14).any()
    cos_small, raw_small = both(lib, small, small_b)
    e, e2 = err(cos_small, sr.cosine_ref(small, small_b)), err(raw_small, sr.normalized_ref(small, small_b))
    print(f"subnormals: cosine {e:.3g}, normalised {e2:.3g}")
    assert e <= BAR and e2 <= BAR


# ------------------------------------------------------------------ special values, once per path
def special_id(c):
    return sr.PATH_NAMES[c[3]]


def rest(x, i, j):
    return np.delete(np.delete(x, i, 0), j, 1)


@pytest.mark.parametrize("case", sr.SPECIAL_SHAPES, ids=special_id)
def test_zero_row_of_a(lib, case):
    """Cosine form: 0 / 0 = NaN across the row, as R:109-114.  Normalised form: 0.0, as F.normalize's clamp (SEG:388)."""
    na, nb, dim, path = case
    assert lib.cosine_gemm_path(na, nb, dim) == path
    a, b = sr.randn_halves(na, nb, dim, seed=2)
    i = na // 2 + 1
    a[i] = 0
    cos, raw = both(lib, a, b)
    assert np.isnan(cos[i]).all()
    assert (raw[i] == 0).all() and not np.isnan(raw).any()
    keep = np.arange(na) != i
    assert err(cos[keep], sr.cosine_ref(a, b)[keep]) <= BAR
    assert err(raw, sr.normalized_ref(a, b)) <= BAR * float(np.linalg.norm(b.astype(np.float64), axis=1).max())


@pytest.mark.parametrize("case", sr.SPECIAL_SHAPES, ids=special_id)
def test_zero_row_of_b(lib, case):
    na, nb, dim, path = case
    assert lib.cosine_gemm_path(na, nb, dim) == path
    a, b = sr.randn_halves(na, nb, dim, seed=3)
    j = nb - 2
    b[j] = 0
    cos, raw = both(lib, a, b)
    assert np.isnan(cos[:, j]).all() and (raw[:, j] == 0).all()
    keep = np.arange(nb) != j
    assert err(cos[:, keep], sr.cosine_ref(a, b)[:, keep]) <= BAR
    assert err(raw, sr.normalized_ref(a, b)) <= BAR * float(np.linalg.norm(b.astype(np.float64), axis=1).max())


@pytest.mark.parametrize("case", sr.SPECIAL_SHAPES, ids=special_id)
def test_non_finite_inputs_stay_in_their_row_and_column(lib, case):
    """One +inf in a row of A, one NaN in a row of B: non-finite exactly there -- nothing leaks through the norm shuffles
    or the LDS reductions."""
    na, nb, dim, path = case
    assert lib.cosine_gemm_path(na, nb, dim) == path
    a, b = sr.randn_halves(na, nb, dim, seed=4)
    clean_cos, clean_raw = sr.cosine_ref(a, b), sr.normalized_ref(a, b)
    i, j = na - 3, nb // 2 + 1
    a[i, dim // 2 + 3] = np.inf
    b[j, dim - 1] = np.nan
    bmax = float(np.linalg.norm(np.delete(b, j, 0).astype(np.float64), axis=1).max())
    for got, exp, bar in zip(both(lib, a, b), (clean_cos, clean_raw), (BAR, BAR * bmax)):
        bad = ~np.isfinite(got)
        want = np.zeros((na, nb), bool)
        want[i], want[:, j] = True, True
        assert np.array_equal(bad, want), np.argwhere(bad != want)[:5]
        assert err(rest(got, i, j), rest(exp, i, j)) <= bar


@pytest.mark.parametrize("case", sr.SPECIAL_SHAPES, ids=special_id)
@pytest.mark.parametrize("entry", ["bff_cosine_gemm_f16", "bff_normalized_gemm_f16"])
def test_bounds(lib, case, entry):
    """The C ABI on operands cut out of the middle of larger buffers whose other rows are NaN, `out` the front of a
    sentinel-filled buffer: all na * nb results written, nothing after them, no neighbour's NaN."""
    na, nb, dim, path = case
    assert lib.cosine_gemm_path(na, nb, dim) == path
    a, b = sr.randn_halves(na, nb, dim, seed=5)
    pad, tail = 3, 1024
    big_a = torch.full((na + 2 * pad, dim), float("nan"), dtype=torch.float16, device=DEV)
    big_b = torch.full((nb + 2 * pad, dim), float("nan"), dtype=torch.float16, device=DEV)
    big_a[pad:pad + na] = dev(a)
    big_b[pad:pad + nb] = dev(b)
    out = torch.full((na * nb + tail,), SENTINEL, dtype=torch.int32, device=DEV)
    lib.call(entry, lib._ptr(big_a[pad:pad + na]), na, lib._ptr(big_b[pad:pad + nb]), nb, dim, lib._ptr(out))
    got = host(out)
    assert (got[na * nb:] == SENTINEL).all()
    assert not (got[:na * nb] == SENTINEL).any()
    res = got[:na * nb].view(np.float32).reshape(na, nb)
    assert np.isfinite(res).all()
    if entry == "bff_cosine_gemm_f16":
        assert err(res, sr.cosine_ref(a, b)) <= BAR
    else:
        assert err(res, sr.normalized_ref(a, b)) <= BAR * float(np.linalg.norm(b.astype(np.float64), axis=1).max())
    assert torch.isnan(big_a[:pad]).all() and torch.isnan(big_b[pad + nb:]).all()          # the operands were only read


def test_gemm_wrappers_refuse_unequal_widths_before_any_launch(lib, monkeypatch):
    """512-d box features against a 768-d bank (box_similarities pads its two arguments independently).  `call` is
    replaced by a stub, so the mismatched read is never launched, whatever the wrappers do."""
    from beyond_fixed_forms_amd import boxfilter
    monkeypatch.setattr(lib, "call", lambda *a, **k: pytest.fail("the library was called with unequal widths"))
    a = torch.zeros(4, 512, dtype=torch.float16, device=DEV)
    b = torch.zeros(3, 768, dtype=torch.float16, device=DEV)
    for fn in (lib.cosine_gemm_f16, lib.normalized_gemm_f16, boxfilter.box_similarities):
        with pytest.raises(ValueError, match="widths differ"):
            fn(a, b)
        with pytest.raises(ValueError, match="widths differ"):
            fn(b, a)


# ------------------------------------------------------------------ the variants, in fresh child processes
def variant_inputs(shape):
    return sr.randn_halves(*shape, seed=6), sr.integer_halves(*shape, seed=7)


def worker(out_path):
    """Every shape of VARIANT_SHAPES through both entry points of this process (switches as inherited) -> one .npz."""
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    out = {}
    for shape in sr.VARIANT_SHAPES:
        key = "x".join(map(str, shape))
        out[key + "_path"] = np.asarray(_lib.cosine_gemm_path(*shape))
        for name, (a, b) in zip(("randn", "int"), variant_inputs(shape)):
            out[f"{key}_{name}_cos"], out[f"{key}_{name}_raw"] = both(_lib, a, b)
    np.savez(out_path, **out)


def test_variants_agree(tmp_path):
    """Default, BFF_GEMM_BANK=0 (the LDS-staged tile64 kernel in the bank kernel's place) and BFF_GEMM_STAGE=4
    (bank<768, 4>), one child after the other; the first that fails ends the test.  Each took its path, is within the bar
    of float64, and on exact integers all three return the same bits."""
    got = {}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for variant, switches in sr.VARIANTS.items():
        path = str(tmp_path / f"{variant}.npz")
        env = {k: v for k, v in os.environ.items() if k not in ("BFF_GEMM_BANK", "BFF_GEMM_STAGE")}
        env.update(switches)
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
        subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, cwd=root, timeout=300)
        got[variant] = np.load(path)
    for shape in sr.VARIANT_SHAPES:
        key = "x".join(map(str, shape))
        (a, b), (ai, bi) = variant_inputs(shape)
        refs = {"randn_cos": sr.cosine_ref(a, b), "randn_raw": sr.normalized_ref(a, b),
                "int_cos": sr.cosine_ref(ai, bi), "int_raw": sr.normalized_ref(ai, bi)}
        bars = {"randn_cos": BAR, "randn_raw": BAR * float(np.linalg.norm(b.astype(np.float64), axis=1).max()),
                "int_cos": BAR, "int_raw": BAR * float(np.linalg.norm(bi.astype(np.float64), axis=1).max())}
        for variant in sr.VARIANTS:
            z = got[variant]
            assert int(z[key + "_path"]) == sr.variant_path(variant, *shape), (variant, shape)
            for name, ref in refs.items():
                assert err(z[f"{key}_{name}"], ref) <= bars[name], (variant, shape, name)
        for name in ("int_cos", "int_raw"):
            first = bits(got["default"][f"{key}_{name}"])
            for variant in ("bank0", "stage4"):
                assert np.array_equal(bits(got[variant][f"{key}_{name}"]), first), (variant, shape, name)
    assert [int(got[v]["2063x200x768_path"]) for v in sr.VARIANTS] == [3, 2, 4]
    assert [int(got[v]["4100x198x512_path"]) for v in sr.VARIANTS] == [5, 2, 5]


# ------------------------------------------------------------------ bff_cosine_rows
# na * nb is no multiple of 4 (the last block's early exit), dim none of 64 but for the CLIP width (the lane guard k < dim)
ROWS_SHAPES = [(1, 1, 1), (3, 5, 7), (7, 3, 100), (5, 9, 1000), (2, 3, 768)]
assert all((na * nb) % 4 for na, nb, _ in ROWS_SHAPES) and sum(dim % 64 != 0 for _, _, dim in ROWS_SHAPES) == 4


def rows_call(lib, a, b):
    """bff_cosine_rows through the C ABI into the front of a sentinel-filled buffer; the tail must stay."""
    na, nb, tail = a.shape[0], b.shape[0], 256
    out = torch.full((na * nb + tail,), SENTINEL, dtype=torch.int32, device=DEV)
    ta, tb = dev(a), dev(b)
    lib.call("bff_cosine_rows", lib._ptr(ta), na, lib._ptr(tb), nb, a.shape[1], 1 if a.dtype == np.float16 else 0,
             lib._ptr(out))
    got = host(out)
    assert (got[na * nb:] == SENTINEL).all() and not (got[:na * nb] == SENTINEL).any()
    res = got[:na * nb].view(np.float32).reshape(na, nb)
    assert np.array_equal(bits(res), bits(host(lib.cosine_rows(ta, tb))))      # the wrapper is the same call
    return res


def rows_inputs(na, nb, dim, dtype):
    rng = np.random.default_rng([na, nb, dim])
    a = rng.standard_normal((na, dim), dtype=np.float32).astype(dtype)
    b = rng.standard_normal((nb, dim), dtype=np.float32).astype(dtype)
    if na > 1:
        a[-1] = a[0]                                          # equal rows must tie exactly
    if nb > 1:
        b[-1] = b[0]
    return a, b


@pytest.mark.parametrize("na,nb,dim", ROWS_SHAPES)
def test_cosine_rows_float32(lib, na, nb, dim):
    a, b = rows_inputs(na, nb, dim, np.float32)
    got = rows_call(lib, a, b)
    e = err(got, sr.cosine_ref(a, b))
    print(f"cosine_rows float32: {e:.3g}")
    assert e <= 5e-7
    assert np.array_equal(bits(got[-1]), bits(got[0])) and np.array_equal(bits(got[:, -1]), bits(got[:, 0]))


@pytest.mark.parametrize("na,nb,dim", ROWS_SHAPES)
def test_cosine_rows_float16(lib, na, nb, dim):
    """Float16 values, within the four half-ulp roundings (2^-10) of the float64 cosine, equal rows tying exactly, and
    equal to the op-by-op rounding of R:109-114 restated in NumPy."""
    a, b = rows_inputs(na, nb, dim, np.float16)
    got = rows_call(lib, a, b)
    assert np.array_equal(got, got.astype(np.float16).astype(np.float32))
    e = err(got, sr.cosine_ref(a, b))
    print(f"cosine_rows float16: {e:.3g}")
    assert e <= 2.0 ** -10
    assert np.array_equal(bits(got[-1]), bits(got[0])) and np.array_equal(bits(got[:, -1]), bits(got[:, 0]))
    assert np.array_equal(got.astype(np.float16), sr.cosine_rows_f16_chain(a, b))


# ------------------------------------------------------------------ bff_description_means
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 768, 2048])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_description_means(lib, dim, dtype):
    """Classes of 1, 2 and 9 rows, a zero row inside the last (F.normalize's clamp: it adds 0 to the mean), an empty
    class between two others (a row of NaN; its neighbours as without it)."""
    desc, offs = sr.description_inputs(dim, np.float32 if dtype == torch.float32 else np.float16)
    desc = torch.from_numpy(desc)
    got = lib.description_means(desc.to(DEV), dev(offs))
    assert got.dtype == dtype and tuple(got.shape) == (4, dim)
    got = host(got.float()).astype(np.float64)
    exp = sr.description_means_ref(desc.numpy(), offs)
    assert np.isnan(got[2]).all() and np.isnan(exp[2]).all()
    keep = [0, 1, 3]
    bar = 1e-4 if dtype == torch.float32 else 2.0 ** -12 + 1e-4   # one float16 rounding of a value <= 1 on top
    e = float(np.abs(got[keep] - exp[keep]).max())
    print(f"description_means {dtype} dim {dim}: {e:.3g}")
    assert np.isfinite(got[keep]).all() and e <= bar
    # without the empty class: the same bits in the other rows
    sub = lib.description_means(desc.to(DEV), dev(np.array([0, 1, 3, 12], np.int32)))
    assert torch.equal(sub.cpu(), lib.description_means(desc.to(DEV), dev(offs)).cpu()[keep])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_description_means_refuses_dim_2049(lib, dtype):
    desc = torch.ones(3, 2049, dtype=dtype, device=DEV)
    offs = dev(np.array([0, 1, 3], np.int32))
    with pytest.raises(RuntimeError, match="dim > 2048"):
        lib.description_means(desc, offs)
    out = torch.full((2 * 2049,), 0x5EA7 if dtype == torch.float16 else SENTINEL,
                     dtype=torch.int16 if dtype == torch.float16 else torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="dim > 2048"):
        lib.call("bff_description_means", lib._ptr(desc), lib._ptr(offs), 2, 2049, 1 if dtype == torch.float16 else 0,
                 lib._ptr(out))
    torch.cuda.synchronize()
    assert (out == (0x5EA7 if dtype == torch.float16 else SENTINEL)).all()  # nothing was launched


if __name__ == "__main__":
    worker(sys.argv[1])
