"""Float64 statements of the similarity kernels (csrc/cosine.hip), the table of shapes their tests run and a restatement
of the rule that picks a GEMM kernel.  NumPy only: nothing here touches the GPU or the library.

Two forms of the matrix-core GEMM (include/bff_hip.h):
  cosine      dot / (|a_i| |b_j|)              compute_clip_similarity, R:109-114: a zero row or column is 0 / 0 = NaN
  normalised  (a_i / max(|a_i|, 1e-12)) . b_j  F.normalize(box_emb) @ text.T, SEG:388-393: a zero row is 0.0"""
import numpy as np

EPS = 1e-12                                                  # F.normalize's clamp

# bff_cosine_gemm_path's answers
SMALL, ROWS, TILE64, BANK768_2, BANK768_4, BANK512 = range(6)
PATH_NAMES = ("small", "rows", "tile64", "bank768x2", "bank768x4", "bank512")


def gemm_path(na, nb, dim, bank=True, stage=2):
    """The dispatch rule restated: bank = BFF_GEMM_BANK is unset or non-zero, stage = BFF_GEMM_STAGE (default 2)."""
    if na <= 0 or nb <= 0 or dim <= 0 or dim % 32:
        return -1
    if nb <= 64:
        return SMALL
    if na < 2048:
        return ROWS
    if nb <= 256 and dim in (768, 512) and bank:
        return BANK512 if dim == 512 else BANK768_2 if stage == 2 else BANK768_4
    return TILE64


# (na, nb, dim, expected path in a process with the default environment)
CASES = [
    (1, 1, 32, SMALL), (16, 16, 32, SMALL),
    (17, 64, 256, SMALL),                                    # exactly one 256-k trip
    (15, 33, 288, SMALL),                                    # one fragment into the second trip
    (33, 64, 1024, SMALL),
    (2050, 64, 768, SMALL),                                  # many rows at the nb = 64 boundary
    (40, 3, 2048, SMALL),
    (1, 65, 32, ROWS),                                       # one k-step: three waves of the block have no work
    (2047, 65, 64, ROWS),                                    # the boundary below tile64
    (16, 208, 96, ROWS),                                     # exactly one 13-tile pass
    (17, 209, 160, ROWS),                                    # a one-tile second pass
    (31, 431, 768, ROWS),                                    # three passes
    (5, 257, 512, ROWS),
    (2048, 65, 32, TILE64),                                  # one step, nothing to prefetch
    (2049, 208, 64, TILE64),
    (2111, 257, 768, TILE64),                                # just past the bank limit
    (2048, 417, 512, TILE64),                                # three passes
    (2100, 200, 736, TILE64),
    (2048, 256, 1024, TILE64),
    (2048, 65, 768, BANK768_2),                              # 5 waves
    (2049, 256, 768, BANK768_2),                             # 16 waves
    (2063, 200, 768, BANK768_2),
    (16400, 65, 768, BANK768_2),                             # 1025 tiles > 4 x 256 blocks: a second round of one tile
    (2048, 66, 512, BANK512),
    (4100, 198, 512, BANK512),
    (16400, 256, 512, BANK512),
]

# the shapes every fresh-process variant (default, BFF_GEMM_BANK=0, BFF_GEMM_STAGE=4) runs
VARIANT_SHAPES = [(2063, 200, 768), (2049, 256, 768), (4100, 198, 512), (16400, 65, 768)]
VARIANTS = {"default": {}, "bank0": {"BFF_GEMM_BANK": "0"}, "stage4": {"BFF_GEMM_STAGE": "4"}}


def variant_path(variant, na, nb, dim):
    return gemm_path(na, nb, dim, bank=variant != "bank0", stage=4 if variant == "stage4" else 2)


# per path the smallest shape of CASES with room for a special row and column next to ordinary ones
SPECIAL_SHAPES = [(16, 16, 32, SMALL), (16, 208, 96, ROWS), (2048, 65, 32, TILE64), (2048, 65, 768, BANK768_2),
                  (2048, 66, 512, BANK512)]


# ------------------------------------------------------------------ inputs
def randn_halves(na, nb, dim, seed=0):
    rng = np.random.default_rng([seed, na, nb, dim])
    return (rng.standard_normal((na, dim), dtype=np.float32).astype(np.float16),
            rng.standard_normal((nb, dim), dtype=np.float32).astype(np.float16))


def spread_bank(b):
    """The bank's rows rescaled to norms spread over 0.25 .. 4 (the normalised form must NOT divide them away)."""
    nb = b.shape[0]
    target = 0.25 * 16.0 ** (np.arange(nb) * 7 % max(nb, 2) / max(nb - 1, 1))
    bd = b.astype(np.float64)
    return (bd * (target / np.linalg.norm(bd, axis=1))[:, None]).astype(np.float16)


def integer_halves(na, nb, dim, seed=1):
    """Integer-valued halves in [-31, 31], A and B drawn differently (asymmetric), no all-zero row: every dot product and
    squared norm is an integer below 2^24 at dim <= 2048 -- exact in float32 in any summation order."""
    rng = np.random.default_rng([seed, na, nb, dim])
    a = rng.integers(-31, 32, (na, dim))
    b = rng.integers(-16, 16, (nb, dim)) * 2 + 1                # odd values only, -31 .. 31
    for m in (a, b):
        while True:
            zero = ~m.any(axis=1)
            if not zero.any():
                break
            m[zero] = rng.integers(-31, 32, (int(zero.sum()), dim))
    return a.astype(np.float16), b.astype(np.float16)


DESCRIPTION_OFFS = np.array([0, 1, 3, 3, 12], np.int32)       # classes of 1, 2, 0 and 9 rows
DESCRIPTION_ZERO_ROW = 6                                     # inside the last class


def description_inputs(dim, dtype, seed=0):
    """(desc [12][dim] in dtype, DESCRIPTION_OFFS).  Every class leans towards a direction of its own, so no mean comes near
    zero (at dim 1 the normalised rows are +-1 and could cancel)."""
    rng = np.random.default_rng([seed, dim])
    offs = DESCRIPTION_OFFS
    desc = rng.standard_normal((12, dim), dtype=np.float32)
    lean = np.sign(rng.standard_normal((4, dim), dtype=np.float32)) * 2
    for c in range(4):
        desc[offs[c]:offs[c + 1]] += lean[c]
    desc[DESCRIPTION_ZERO_ROW] = 0
    return desc.astype(dtype), offs


# ------------------------------------------------------------------ float64 statements
def cosine_ref(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (a @ b.T) / (np.linalg.norm(a, axis=1)[:, None] * np.linalg.norm(b, axis=1)[None, :])


def normalize_ref(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), EPS)


def normalized_ref(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return normalize_ref(a) @ np.asarray(b, np.float64).T


def description_means_ref(desc, offs):
    """normalize(mean(normalize(rows))) per class; an empty class is a row of NaN."""
    desc = np.asarray(desc, np.float64)
    out = np.full((len(offs) - 1, desc.shape[1]), np.nan)
    unit = normalize_ref(desc)
    for c in range(len(offs) - 1):
        if offs[c + 1] > offs[c]:
            m = unit[offs[c]:offs[c + 1]].mean(axis=0)
            with np.errstate(invalid="ignore", divide="ignore"):
                out[c] = m / np.linalg.norm(m)
    return out


def exact_bits(a, b):
    """The float32 (cosine form, normalised form) every GEMM kernel must return, bit for bit, on integer_halves: the
    integer sums are exact, what is left is float32 square roots, one product and one quotient, all correctly rounded."""
    ad, bd = a.astype(np.float64), b.astype(np.float64)
    acc, sa, sb = ad @ bd.T, (ad * ad).sum(1), (bd * bd).sum(1)
    assert np.abs(acc).max() < 2 ** 24 and sa.max() < 2 ** 24 and sb.max() < 2 ** 24
    acc, na_ = acc.astype(np.float32), np.sqrt(sa.astype(np.float32))
    return acc / (na_[:, None] * np.sqrt(sb.astype(np.float32))[None, :]), acc / na_[:, None]


def cosine_rows_f16_chain(a, b):
    """bff_cosine_rows on float16 rows: (e1 @ e2.T) / (e1.norm() * e2.norm().T) with every tensor op rounded to float16
    (the sums themselves in float64, rounded through float32 as the kernel does)."""
    ad, bd = a.astype(np.float64), b.astype(np.float64)
    h = lambda x: x.astype(np.float32).astype(np.float16)
    hd = h(ad @ bd.T)
    h1, h2 = h(np.sqrt((ad * ad).sum(1))), h(np.sqrt((bd * bd).sum(1)))
    den = (h1.astype(np.float32)[:, None] * h2.astype(np.float32)[None, :]).astype(np.float16)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (hd.astype(np.float32) / den.astype(np.float32)).astype(np.float16)
