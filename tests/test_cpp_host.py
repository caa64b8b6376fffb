"""The C++ host mirror of internal/rs and internal/rs/gf (include/slime_rs.hpp)
through its own parity program (tests/cpp/rs_host_test.cpp, built by `make`):
the reference's Go tests restated in C++ against the committed fixtures.
Host-only cases run here; data-path cases need the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "rs_host_test")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _run(group: str) -> str:
    if not os.path.exists(BIN):  # built by `make` / __graft_entry__.build()
        subprocess.run(["make", "-C", ROOT, "tests/cpp/rs_host_test"], check=True, capture_output=True)
    r = subprocess.run([BIN, GOLDEN, group], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout
    return r.stdout


def test_cpp_host_mirror_host_only():
    out = _run("cpu")
    for name in ("TestVandermonde", "TestParityMatrix", "TestParityMatrixInvertible", "TestMInverse",
                 "TestValidationPanics", "TestCallDetailPerCall", "TestWriteChunksConfigChecks"):
        assert f"ok   {name}" in out


@pytest.mark.gpu
def test_cpp_host_mirror_data_path():
    out = _run("gpu")
    for name in ("TestCreateParity", "TestRecovery", "TestMapTrivial", "TestMapTricky", "TestWriteChunksRoundTrip",
                 "TestWriteChunksNoParity", "TestDevicePool", "TestWriteChunksDigest"):
        assert f"ok   {name}" in out


CACHE_BIN = os.path.join(ROOT, "tests", "cpp", "plan_cache_test")


def test_plan_cache_is_bounded_and_safe_under_eviction():
    """slime_amd/csrc/plan_cache.hpp over the product's host matrix code:
    10,000 distinct 20/40 survivor sets keep the live plan count at the cap
    and release every evicted table; held plans survive concurrent eviction;
    builds run outside the cache lock (8 slow builds of different keys
    overlap, one key's concurrent callers share one build) and evicted plans
    are released after it is dropped."""
    subprocess.run(["make", "-C", ROOT, "tests/cpp/plan_cache_test"], check=True, capture_output=True)
    r = subprocess.run([CACHE_BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("TestPlanCacheBounded", "TestPlanCacheFailedBuild", "TestPlanCacheConcurrent",
                 "TestPlanCacheBuildsOutsideLock", "TestPlanCacheSharedBuild", "TestPlanCacheReleaseOutsideLock"):
        assert f"ok   {name}" in r.stdout


COPY_BIN = os.path.join(ROOT, "tests", "cpp", "copy_pool_test")


@pytest.mark.parametrize("threads", ["0", "4"])
def test_copy_pool_under_concurrent_callers(threads):
    """host_copy.cpp: 8 callers x 60 jobs of 1-5 items (tiny to 6 MiB, odd
    offsets) land byte-exact with nothing written around them, with no pool
    workers and with 4."""
    if not os.path.exists(COPY_BIN):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/copy_pool_test"], check=True, capture_output=True)
    env = dict(os.environ, SLIME_RS_COPY_THREADS=threads)
    r = subprocess.run([COPY_BIN], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout



POOL_BIN = os.path.join(ROOT, "tests", "cpp", "device_pool_test")


def test_device_pool_routing_with_a_fixed_device_count():
    """device_pool.hpp (the routing rs_capi.cpp uses) on 8 stand-in devices:
    25 concurrent callers spread within 40% of an even share (the bound holds
    on a CPU the suite's parallel workers share), every workspace and plan a
    call gets is its device's, pinned devices (per call, per thread,
    SLIME_RS_DEVICES) are honoured, and the least-loaded device wins."""
    subprocess.run(["make", "-C", ROOT, "tests/cpp/device_pool_test"], check=True, capture_output=True)
    r = subprocess.run([POOL_BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("TestAllowedDevices", "TestPoolSpreadsConcurrentCallers", "TestPinnedDevices", "TestLeastLoaded",
                 "TestHostCallSlotsFifo"):
        assert f"ok   {name}" in r.stdout


MFMA_BIN = os.path.join(ROOT, "tests", "cpp", "mfma_table_test")


def test_mfma_table_arithmetic_emulated():
    """The matrix-core kernel's exact int8-limb identity (mfma_table.hpp),
    emulated on the CPU from the very A-fragment table a plan uploads and the
    B fragments the kernel assembles: every (rows, k) shape the kernel takes
    (k up to 112, rows up to 32, symbol and big-endian byte order) is
    bit-exact against sum_j c_ij x_j mod p, including non-canonical symbols
    and coefficients at the digit window's edges."""
    subprocess.run(["make", "-C", ROOT, "tests/cpp/mfma_table_test"], check=True, capture_output=True)
    r = subprocess.run([MFMA_BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bit-exact" in r.stdout
    assert "saturated cases at k=112, largest |D_e| = " in r.stdout


FOLD_BIN = os.path.join(ROOT, "tests", "cpp", "gfp_fold_test")


def test_fold96_against_int128_at_its_rare_branches():
    """fold96 (gfp.hpp), the last step of every data kernel, compiled for the
    host and compared with unsigned __int128 % p: V = q p + t and
    q 2^32 + t - d around every limb boundary for hi = 0..300, the matrix-core
    range (hi = 0, lo < 2^49), every (lo, hi) of edge limbs, 10^7 random
    values.  The program itself refuses a value set that never takes
    `u >> 32 == 1` or the final `w >= p`."""
    subprocess.run(["make", "-C", ROOT, "tests/cpp/gfp_fold_test"], check=True, capture_output=True)
    r = subprocess.run([FOLD_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "10000000 random bit-exact" in r.stdout


DMA_BIN = os.path.join(ROOT, "tests", "cpp", "dma_plan_test")


def test_dma_plan_extents_are_checked():
    """slime_amd/csrc/dma_plan.hpp (the copies dma_spans issues): host_apply's
    and write_chunks' window layouts plan to the expected pitched / blit
    commands whose last byte is the last span's; 3000 random span lists
    replayed byte by byte copy exactly their spans and nothing else; the
    extent check refuses a plan one byte past either buffer and a pitched
    extent that overflows 64 bits (the bound on every
    hipMemcpy2DAsync / hipMemcpyAsync extent)."""
    subprocess.run(["make", "-C", ROOT, "tests/cpp/dma_plan_test"], check=True, capture_output=True)
    r = subprocess.run([DMA_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("TestHostApplyLayout", "TestWriteChunksLayout", "TestPlanFaithful", "TestExtentOverflow"):
        assert f"ok   {name}" in r.stdout


REDO_BIN = os.path.join(ROOT, "tests", "cpp", "redo_list_test")


def test_redo_list_counter_protocol_emulated():
    """slime_amd/csrc/redo_list.hpp (the matrix-core redo list's counter word,
    rs_bytes_mfma.hip): waves setting the switched bit before and after
    others draw offsets, in every fixed order and on 8 real threads over 60
    random batches -- every drawn offset masked, each needed entry listed
    once, the count and the switched flag recovered; redo_list_fits refuses
    batches of 2^31 entries or more, which then take the whole-object redo
    (VERDICT r05 item 2)."""
    subprocess.run(["make", "-C", ROOT, "tests/cpp/redo_list_test"], check=True, capture_output=True)
    r = subprocess.run([REDO_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("TestRedoListFixedOrders", "TestRedoListConcurrent", "TestRedoListFits"):
        assert f"ok   {name}" in r.stdout


PROBE_BIN = os.path.join(ROOT, "tests", "cpp", "probe_layout_test")


def test_probe_layout_keeps_the_table_aligned_and_inside():
    """slime_amd/csrc/probe_layout.hpp (where placement_probe puts its table):
    for every bytes % 256 residue, around 402 MB, 512 MiB and 16 GiB +- 3, the
    table's offset is a multiple of 256, the table ends inside the range, the
    objects end at or before it and L is a multiple of 64; too-small ranges are
    refused (L == 0).  The kernels read the table with scalar loads, which
    ignore the low address bits: a table at `bytes - 4096` of an odd-sized
    range shifted the shard indices and sent the walk outside the buffer."""
    subprocess.run(["make", "-C", ROOT, "tests/cpp/probe_layout_test"], check=True, capture_output=True)
    r = subprocess.run([PROBE_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("TestEveryResidue", "TestAroundTheSizesCallersUse", "TestRefusals"):
        assert f"ok   {name}" in r.stdout
