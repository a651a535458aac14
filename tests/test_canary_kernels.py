"""The canary kernels (gpushare_amd/native/canary.hip) against independent
references.

probe() judges itself: its write and check kernels share one formula, its
MFMA reference sits next to the launch, its copy was only timed.  These
tests hold each kernel against a reference computed here, in numpy — the
VRAM pattern in uint64 wrap-around arithmetic, the MFMA tile in float64 —
and show that the probe can say "no": a corrupted word is counted exactly
once, a mutated tile is a mismatch, a probe of nothing is an error.

Nothing here imports gpushare_amd._canary; tests/canary_cases.py runs every
case in one fresh torch-free child per group (one CPU child, one GPU child)
and the tests assert on what it wrote.  A child that fails or times out
fails every test of its group.
"""

import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import canary_cases as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULT = 0x9E3779B97F4A7C15
U = 2.0 ** -24                      # float32 unit roundoff
GAMMA4 = 4 * U / (1 - 4 * U)        # length-4 dot product, any order


def _built():
    return bool(glob.glob(os.path.join(REPO, "gpushare_amd", "_canary*.so")))


def _run_child(mode, outdir, timeout):
    cmd = [sys.executable, os.path.join(REPO, "tests", "canary_cases.py"),
           mode, str(outdir)]
    try:
        proc = subprocess.run(cmd, capture_output=True, text=True,
                              timeout=timeout, cwd=REPO)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"canary_cases {mode} timed out after {timeout}s: "
                    f"{(e.stderr or b'')[-2000:]!r}")
    if proc.returncode != 0:
        pytest.fail(f"canary_cases {mode} rc={proc.returncode}\n"
                    f"{proc.stderr[-4000:]}")
    with open(os.path.join(outdir, "results.json")) as f:
        res = json.load(f)
    with np.load(os.path.join(outdir, "arrays.npz")) as z:
        arr = {k: z[k] for k in z.files}
    return res, arr


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    if not _built():
        pytest.skip("_canary extension not built")
    return _run_child("cpu", tmp_path_factory.mktemp("canary_cpu"), 60)


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    assert _built(), "_canary extension not built"
    return _run_child("gpu", tmp_path_factory.mktemp("canary_gpu"), 120)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pattern(n, seed):
    """The walk's pattern, independently: uint64 wrap-around in numpy."""
    with np.errstate(over="ignore"):
        return np.uint64(seed) ^ (np.arange(n, dtype=np.uint64) * np.uint64(MULT))


def once_rounded(A, B):
    """float32(A·B) through float64.  Exact when every output is a single
    product (a 48-bit product fits float64), or exactly representable."""
    return (A.astype(np.float64) @ B.astype(np.float64)).astype(np.float32)


# --------------------------------------------------------------------------- #
# CPU group: host-only entry points, no GPU needed
# --------------------------------------------------------------------------- #

def test_stock_reference_is_exact_float64_product(cpu):
    _, arr = cpu
    A, B, ref = arr["stock_A"], arr["stock_B"], arr["stock_ref"]
    exact = A.astype(np.float64) @ B.astype(np.float64)
    # small dyadic operands: every partial sum is representable
    assert np.array_equal(ref.astype(np.float64), exact)
    assert not np.isnan(ref).any()
    assert np.array_equal(bits(ref), bits(exact.astype(np.float32)))


def test_full_mantissa_operands_and_reference(cpu):
    """The probe's second tile: one product per output, so its host chain
    must be the once-rounded float64 product; and the operands must really
    toggle every fraction bit, inside the magnitude range the GPU tests
    assume."""
    _, arr = cpu
    A, B, ref = arr["full_A"], arr["full_B"], arr["full_ref"]
    assert np.count_nonzero(A) == 16 and np.count_nonzero(B) == 64
    for r in range(16):
        assert A[r, r % 4] != 0
    assert np.array_equal(bits(ref), bits(once_rounded(A, B)))
    for vals in (A[A != 0], B.ravel()):
        assert (np.abs(vals) >= 2.0 ** -8).all() and (np.abs(vals) < 2.0 ** 8).all()
        frac = bits(vals) & np.uint32(0x7FFFFF)
        assert np.bitwise_or.reduce(frac) == 0x7FFFFF    # each bit set somewhere
        assert np.bitwise_and.reduce(frac) == 0          # and clear somewhere
    # the 256 products exercise every result fraction bit both ways too
    frac = bits(ref) & np.uint32(0x7FFFFF)
    assert np.bitwise_or.reduce(frac.ravel()) == 0x7FFFFF
    assert np.bitwise_and.reduce(frac.ravel()) == 0


def test_judge_accepts_identity(cpu):
    res, _ = cpu
    assert res["self_mismatches"] == 0


@pytest.mark.parametrize(
    "mutation",
    ["transposed", "rows_swapped", "cols_swapped", "block_map", "one_ulp", "nan"],
)
def test_judge_catches_mutation(cpu, mutation):
    """The stock operands are not symmetric under the mistakes the probe
    claims to catch."""
    res, arr = cpu
    # the mutation really changes the tile (else the case proves nothing)
    mutated = cc.mutations(arr["stock_ref"])[mutation]
    assert not np.array_equal(bits(mutated), bits(arr["stock_ref"]))
    assert res["mutations"][mutation] > 0


def test_pattern_word_matches_python_integers(cpu):
    """pattern_word against unbounded Python integers, including indices
    past 2**32.  The kernels share this expression, but their 64-bit index
    arithmetic cannot be checked on the GPU without a buffer over 32 GiB;
    that GPU check is out of scope."""
    res, _ = cpu
    seen = set()
    for i, seed, got in res["pattern"]:
        assert got == seed ^ ((i * MULT) % 2**64), (i, seed)
        seen.add(i)
    assert seen == {0, 1, 2**32 - 1, 2**32, 2**40 + 3}


def test_argument_validation_raises_before_hip(cpu):
    """A probe or walk over nothing must be an error, not a healthy verdict;
    the ValueError comes before any HIP call, so it shows on a GPU-less
    host (where a HIP call would give RuntimeError instead)."""
    res, _ = cpu
    assert res["validation"] == {k: "ValueError" for k in res["validation"]}
    assert {"probe_mb_0", "probe_mb_neg", "walk_n_0", "walk_n_neg"} <= set(
        res["validation"])


def test_health_monitor_rejects_empty_probe_span():
    from gpushare_amd.health import HealthMonitor

    for mb in (0, -1):
        with pytest.raises(ValueError):
            HealthMonitor(None, None, deep_probe_interval=1.0, probe_vram_mb=mb)
    HealthMonitor(None, None, deep_probe_interval=1.0, probe_vram_mb=1)


# --------------------------------------------------------------------------- #
# GPU group
# --------------------------------------------------------------------------- #

@pytest.mark.gpu
@pytest.mark.parametrize("k", range(4))
def test_mfma_lane_mapping_exact(gpu, k):
    """Column k of A (distinct integers) times row k of B (distinct primes):
    all 256 products differ, so C equals the outer product only if the A, B
    and C lane maps are right for every lane of this k-group."""
    _, arr = gpu
    A, B = cc.mfma_cases()[f"lanes_k{k}"]
    expect = once_rounded(A, B)
    assert len(np.unique(np.abs(expect))) == 256
    assert np.array_equal(bits(arr[f"mfma_lanes_k{k}"]), bits(expect))


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(4))
def test_mfma_full_mantissa_exact(gpu, k):
    """One product per output from 24-bit-significand operands: one correct
    rounding, fused or not, so the result is float32(float64(a)*float64(b))
    bit for bit."""
    _, arr = gpu
    A, B = cc.mfma_cases()[f"mantissa_k{k}"]
    assert np.array_equal(bits(arr[f"mfma_mantissa_k{k}"]), bits(once_rounded(A, B)))


@pytest.mark.gpu
def test_mfma_dense_within_dot_product_bound(gpu):
    """Dense full-mantissa operands against float64 A·B.  The bound
    gamma_4·(|A|·|B|), gamma_4 = 4u/(1-4u), u = 2**-24, is the standard
    length-4 dot-product bound; it holds for any accumulation order, fused
    or not.  Derived, not measured."""
    _, arr = gpu
    A, B = cc.mfma_cases()["dense"]
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    ref = A64 @ B64
    bound = GAMMA4 * (np.abs(A64) @ np.abs(B64))
    # the reference's own rounding to float32 sits inside the bound
    assert (np.abs(ref.astype(np.float32).astype(np.float64) - ref) <= bound).all()
    C = arr["mfma_dense"].astype(np.float64)
    err = np.abs(C - ref)
    print("dense max err/bound:", float((err / bound).max()))
    assert (err <= bound).all()


@pytest.mark.gpu
def test_mfma_stock_tile_bitwise(gpu):
    _, arr = gpu
    assert np.array_equal(bits(arr["stock_C"]), bits(arr["stock_ref"]))
    # and against float64, independently of the extension's host chain
    exact = arr["stock_A"].astype(np.float64) @ arr["stock_B"].astype(np.float64)
    assert np.array_equal(arr["stock_C"].reshape(16, 16).astype(np.float64), exact)


@pytest.mark.gpu
def test_mfma_probe_full_mantissa_tile_bitwise(gpu):
    """The second tile probe() judges: kernel output == host chain == the
    once-rounded float64 product."""
    _, arr = gpu
    expect = once_rounded(arr["full_A"], arr["full_B"]).ravel()
    assert np.array_equal(bits(arr["full_C"]), bits(expect))
    assert np.array_equal(bits(arr["full_C"]), bits(arr["full_ref"]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", cc.TAIL_CASES, ids=[c[0] for c in cc.TAIL_CASES])
def test_vram_walk_writes_independent_pattern(gpu, case):
    """Grid-stride tails: sizes around one block, one grid and a ragged end,
    on the production grid and a tiny one.  The dumped buffer must equal the
    numpy pattern word for word and leave the guard words alone."""
    name, n, _, _ = case
    res, arr = gpu
    buf = arr[f"walk_{name}"]
    assert buf.shape == (n + cc.GUARD,)
    assert np.array_equal(buf[:n], pattern(n, cc.SEED))
    assert (buf[n:] == np.uint64(0xCDCDCDCDCDCDCDCD)).all()
    assert res["tails"][name] == {"mismatches": 0, "guard_intact": True}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(cc.detect_cases()))
def test_vram_check_counts_corruption_exactly(gpu, case):
    """Valid launches over data the test changed: one corrupted word is one
    mismatch (first, last, either side of the grid-stride seam; one bit or
    all), five are five, and a corrupted guard word is none — the check
    stops at n."""
    res, _ = gpu
    corrupt, expected = cc.detect_cases()[case]
    got = res["detect"][case]
    assert got["mismatches"] == expected
    in_guard = any(i >= cc.DETECT_N for i, _ in corrupt)
    assert got["guard_intact"] == (not in_guard)


@pytest.mark.gpu
def test_vram_pattern_depends_on_seed(gpu):
    _, arr = gpu
    n = 2 * cc.T + 17
    buf = arr[f"walk_prod_{n}"][:n]
    assert (buf != pattern(n, cc.SEED ^ 1)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n4", cc.COPY_N4)
def test_bw_copy_copies_everything_and_no_more(gpu, n4):
    """dst starts sentinel-filled, so a copy that stops short shows as
    mismatches and one that runs long breaks the guard."""
    res, _ = gpu
    assert res["copy"][str(n4)] == {"mismatches": 0, "guard_intact": True}


@pytest.mark.gpu
def test_probe_twice_verifies_copy_and_serialises(gpu):
    res, _ = gpu
    assert len(res["probes"]) == 2
    for r in res["probes"]:
        assert r["ok"] and r["mfma_ok"] and r["vram_ok"], r
        assert r["mfma_mismatches"] == 0 and r["vram_mismatches"] == 0
        assert r["hbm_copy_mismatches"] == 0
        assert r["vram_probed_bytes"] == 1 << 20
    assert json.loads(res["probes_json"]) == res["probes"]
