"""Child-process runner for tests/test_canary_kernels.py.

The pytest process must never import gpushare_amd._canary (torch's bundled
libamdhip64 and the system one conflict by load order, and
test_lifecycle.py asserts the extension stays out of sys.modules), so every
call into the extension happens here, in one fresh torch-free process per
group:

    python tests/canary_cases.py cpu OUTDIR    # host-only entry points
    python tests/canary_cases.py gpu OUTDIR    # kernels on device 0

Each run writes OUTDIR/results.json (scalars) and OUTDIR/arrays.npz.  This
file only produces inputs and raw outputs; every reference and every
assertion lives in the parent.  The input builders below are imported by
the parent too, so both sides see the same operands.
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

T = 2048 * 256       # threads of the production walk grid
T_TINY = 4 * 256     # threads of the tiny walk grid
T4 = 4096 * 256      # threads of the production copy grid
GUARD = 64
SEED = 0x0123456789ABCDEF
FULL = 0xFFFFFFFFFFFFFFFF
PATTERN_INDICES = [0, 1, 2**32 - 1, 2**32, 2**40 + 3]
PATTERN_SEEDS = [0, SEED, FULL]

# (name, n_words, grid, block): every size at which the grid-stride loops
# take another path — below/at/above one block, one grid, and a ragged tail
TAIL_CASES = [
    (f"prod_{n}", n, 2048, 256)
    for n in (1, 255, 256, 257, T - 1, T, T + 1, 2 * T + 17)
] + [
    (f"tiny_{n}", n, 4, 256)
    for n in (1, T_TINY - 1, T_TINY, T_TINY + 1, 3 * T_TINY + 5)
]

DETECT_N = T + 5     # index T is inside the buffer and on a second trip


def detect_cases():
    """name -> (corrupt list, expected mismatches); n = DETECT_N, GUARD guard
    words, production grid."""
    n = DETECT_N
    cases = {}
    for where, idx in (("first", 0), ("last", n - 1), ("Tm1", T - 1), ("T", T)):
        for mname, mask in (("bit0", 1), ("bit63", 1 << 63), ("full", FULL)):
            cases[f"{where}_{mname}"] = ([(idx, mask)], 1)
    cases["scattered5"] = (
        [(3, 1 << 17), (T - 2, FULL), (T + 1, 1 << 40), (n // 2, 2), (n - 2, 1 << 62)],
        5,
    )
    # words past n: the check must stop at n
    cases["guard_first"] = ([(n, FULL)], 0)
    cases["guard_last"] = ([(n + GUARD - 1, 1)], 0)
    return cases


COPY_N4 = [1, T4 - 1, T4, T4 + 1, 2 * T4 + 3]


def _full_mantissa(rng, count):
    """Normal float32s with random sign, exponent in [-8, 7] and 23 random
    fraction bits: magnitude in [2**-8, 2**8)."""
    sign = rng.integers(0, 2, count, dtype=np.uint32) << np.uint32(31)
    expo = (rng.integers(-8, 8, count) + 127).astype(np.uint32) << np.uint32(23)
    frac = rng.integers(0, 1 << 23, count, dtype=np.uint32)
    return (sign | expo | frac).view(np.float32)


PRIMES = [17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79]


def mfma_cases():
    """name -> (A[16,4], B[4,16]) float32.  One-hot-k cases leave everything
    but column k of A and row k of B at zero, so each output is one product.
    """
    cases = {}
    rng = np.random.default_rng(0xC0FFEE)
    for k in range(4):
        # distinct integers 1..16 (permuted, signed) times distinct primes
        # above 16: every one of the 256 products is unique in magnitude
        A = np.zeros((16, 4), np.float32)
        B = np.zeros((4, 16), np.float32)
        r = np.arange(16)
        A[:, k] = ((r * 5 + k * 3) % 16 + 1) * np.where((r + k) % 2, -1.0, 1.0)
        B[k, :] = np.roll(PRIMES, k)
        cases[f"lanes_k{k}"] = (A, B)
    for k in range(4):
        A = np.zeros((16, 4), np.float32)
        B = np.zeros((4, 16), np.float32)
        A[:, k] = _full_mantissa(rng, 16)
        B[k, :] = _full_mantissa(rng, 16)
        cases[f"mantissa_k{k}"] = (A, B)
    cases["dense"] = (
        _full_mantissa(rng, 64).reshape(16, 4),
        _full_mantissa(rng, 64).reshape(4, 16),
    )
    return cases


def mutations(ref):
    """name -> a wrong 16x16 result the probe's judge claims to catch."""
    ref = ref.reshape(16, 16)
    out = {"transposed": ref.T.copy()}
    rows = ref.copy()
    rows[[2, 9]] = rows[[9, 2]]
    out["rows_swapped"] = rows
    cols = ref.copy()
    cols[:, [0, 15]] = cols[:, [15, 0]]
    out["cols_swapped"] = cols
    # C/D register map (l/16)*4+i mistaken for i*4 + l/16
    block = np.empty_like(ref)
    for j in range(4):
        for i in range(4):
            block[i * 4 + j] = ref[j * 4 + i]
    out["block_map"] = block
    ulp = ref.copy()
    ulp[7, 3] = np.nextafter(ulp[7, 3], np.float32(np.inf))
    out["one_ulp"] = ulp
    nan = ref.copy()
    nan[11, 5] = np.nan
    out["nan"] = nan
    return out


def _flat(a):
    return np.asarray(a, np.float32).ravel().tolist()


def _raises(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001
        return type(e).__name__
    return None


def run_cpu(canary):
    res, arr = {}, {}
    for name, fn in (("stock", canary.stock_operands),
                     ("full", canary.full_mantissa_operands)):
        A, B = fn()
        ref = canary.mfma_reference(A, B)
        arr[f"{name}_A"] = np.array(A, np.float32).reshape(16, 4)
        arr[f"{name}_B"] = np.array(B, np.float32).reshape(4, 16)
        arr[f"{name}_ref"] = np.array(ref, np.float32).reshape(16, 16)
    ref = arr["stock_ref"]
    res["self_mismatches"] = canary.count_mismatches(_flat(ref), _flat(ref))
    res["mutations"] = {
        name: canary.count_mismatches(_flat(m), _flat(ref))
        for name, m in mutations(ref).items()
    }
    res["pattern"] = [
        [i, s, canary.pattern_word(i, s)]
        for i in PATTERN_INDICES for s in PATTERN_SEEDS
    ]
    # argument validation must fire before any HIP call (no GPU needed)
    res["validation"] = {
        "probe_mb_0": _raises(lambda: canary.probe(0, vram_probe_mb=0)),
        "probe_mb_neg": _raises(lambda: canary.probe(0, vram_probe_mb=-1)),
        "probe_mb_neg_bw": _raises(lambda: canary.probe(0, -64, True)),
        "walk_n_0": _raises(lambda: canary.vram_walk(0, 0, SEED)),
        "walk_n_neg": _raises(lambda: canary.vram_walk(0, -8, SEED)),
        "walk_corrupt_oob": _raises(
            lambda: canary.vram_walk(0, 4, SEED, guard_words=2, corrupt=[(6, 1)])
        ),
        "walk_grid_0": _raises(lambda: canary.vram_walk(0, 4, SEED, grid=0)),
        "copy_n4_0": _raises(lambda: canary.copy_walk(0, 0)),
        "tile_short": _raises(lambda: canary.mfma_tile(0, [1.0] * 63, [1.0] * 64)),
    }
    return res, arr


def run_gpu(canary):
    res, arr = {}, {}
    assert canary.device_count() >= 1, "no GPU visible"

    for name, (A, B) in mfma_cases().items():
        C = canary.mfma_tile(0, _flat(A), _flat(B))
        arr[f"mfma_{name}"] = np.array(C, np.float32).reshape(16, 16)
    for name, fn in (("stock", canary.stock_operands),
                     ("full", canary.full_mantissa_operands)):
        A, B = fn()
        arr[f"{name}_A"] = np.array(A, np.float32).reshape(16, 4)
        arr[f"{name}_B"] = np.array(B, np.float32).reshape(4, 16)
        arr[f"{name}_ref"] = np.array(canary.mfma_reference(A, B), np.float32)
        arr[f"{name}_C"] = np.array(canary.mfma_tile(0, A, B), np.float32)

    res["tails"] = {}
    for name, n, grid, block in TAIL_CASES:
        r = canary.vram_walk(0, n, SEED, grid=grid, block=block,
                             guard_words=GUARD, dump=True)
        arr[f"walk_{name}"] = np.frombuffer(r.pop("buffer"), np.uint64)
        res["tails"][name] = r

    res["detect"] = {}
    for name, (corrupt, _) in detect_cases().items():
        res["detect"][name] = canary.vram_walk(
            0, DETECT_N, SEED, guard_words=GUARD, corrupt=corrupt)

    res["copy"] = {str(n4): canary.copy_walk(0, n4, guard_words=GUARD)
                   for n4 in COPY_N4}

    # two probes back to back: the second runs on whatever the first freed
    res["probes"] = [canary.probe(0, vram_probe_mb=1, bandwidth=True)
                     for _ in range(2)]
    res["probes_json"] = json.dumps(res["probes"])
    return res, arr


def main(argv):
    mode, outdir = argv
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gpushare_amd._canary as canary

    res, arr = {"cpu": run_cpu, "gpu": run_gpu}[mode](canary)
    np.savez(os.path.join(outdir, "arrays.npz"), **arr)
    with open(os.path.join(outdir, "results.json"), "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
