// gpushare_amd._canary — deep GPU health probe for MI355X (gfx950).
//
// The reference's health model is passive: it waits for NVML XID events
// (reference: pkg/gpu/nvidia/nvidia.go:100-152).  On a shared GPU a passive
// watcher misses the failure mode that matters most to co-located tenants —
// a GPU that still enumerates but no longer executes correctly.  This probe
// actively verifies, in a few milliseconds, that:
//   1. the command processor accepts and completes kernel launches,
//   2. the MFMA matrix cores produce bit-exact results
//      (v_mfma_f32_16x16x4_f32 is exact fp32 per the CDNA4 ISA), on a
//      stock tile (lane mapping) and a full-mantissa tile (every bit),
//   3. a VRAM span can be written and read back intact,
//   4. HBM3E delivers sane streaming bandwidth (reported, not judged) and
//      the streamed copy arrives intact (judged).
//
// probe() is assembled from the smaller entry points exported below
// (mfma_tile, vram_walk, copy_walk and the host-only judges), so that
// tests/test_canary_kernels.py can hold each kernel against an independent
// reference instead of against itself.
//
// Used by the health watcher (gpushare_amd/health.py) alongside the passive
// amdsmi event stream, and by __graft_entry__.smoke() / pytest -m gpu.
//
// Build: hipcc --offload-arch=gfx950 (see gpushare_amd/native/build.py).

#include <hip/hip_runtime.h>

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace py = pybind11;

#define HIP_CHECK(expr)                                                    \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    if (_e != hipSuccess)                                                  \
      throw std::runtime_error(std::string("HIP error at " #expr ": ") +   \
                               hipGetErrorString(_e));                     \
  } while (0)

namespace {

// ---------------------------------------------------------------------------
// Kernel 1: MFMA canary.  One wavefront computes C = A·B for a 16×16 tile
// (K=4) with v_mfma_f32_16x16x4_f32.  Exact fp32 → host-verifiable
// bit-for-bit.  Lane mapping (CDNA4 ISA):
//   A (16×4): lane l holds A[l%16][l/16]
//   B (4×16): lane l holds B[l/16][l%16]
//   C/D (16×16): lane l, reg i → C[(l/16)*4 + i][l%16]
// ---------------------------------------------------------------------------

using f32x4 = __attribute__((ext_vector_type(4))) float;

__global__ void mfma_canary_kernel(const float *__restrict__ A,
                                   const float *__restrict__ B,
                                   float *__restrict__ C) {
#if defined(__gfx950__)
  int lane = threadIdx.x;  // single wavefront of 64
  float a = A[(lane % 16) * 4 + (lane / 16)];
  float b = B[(lane / 16) * 16 + (lane % 16)];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    C[((lane / 16) * 4 + i) * 16 + (lane % 16)] = acc[i];
#else
  // Non-gfx950 build: poison the output so the probe fails loudly rather
  // than silently passing on the wrong architecture.
  if (threadIdx.x == 0) C[0] = -1.0f / 0.0f;
#endif
}

// ---------------------------------------------------------------------------
// Kernel 2: VRAM pattern walk.  Writes an address-derived pattern and a
// second kernel verifies it, accumulating a mismatch count.  Touches `n`
// uint64s spread across the allocation.
// ---------------------------------------------------------------------------

__host__ __device__ inline uint64_t pattern_at(size_t i, uint64_t seed) {
  return seed ^ (i * 0x9e3779b97f4a7c15ull);
}

__global__ void vram_write_pattern(uint64_t *buf, size_t n, uint64_t seed) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = gridDim.x * (size_t)blockDim.x;
  for (; i < n; i += stride) buf[i] = pattern_at(i, seed);
}

__global__ void vram_check_pattern(const uint64_t *buf, size_t n,
                                   uint64_t seed,
                                   unsigned long long *mismatches) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = gridDim.x * (size_t)blockDim.x;
  unsigned long long bad = 0;
  for (; i < n; i += stride)
    if (buf[i] != pattern_at(i, seed)) ++bad;
  if (bad) atomicAdd(mismatches, bad);
}

// ---------------------------------------------------------------------------
// Kernel 3: streaming-copy bandwidth probe (float4 loads/stores; grid sized
// ≫256 workgroups so all 8 XCDs fill).
// ---------------------------------------------------------------------------

__global__ void bw_copy(const float4 *__restrict__ src, float4 *__restrict__ dst,
                        size_t n4) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = gridDim.x * (size_t)blockDim.x;
  for (; i < n4; i += stride) dst[i] = src[i];
}

// ---------------------------------------------------------------------------
// Host side.  Device buffers and events are owned by RAII holders so that a
// HIP_CHECK throw on any path releases them (an in-process daemon probes
// every interval; a failing GPU must not also leak VRAM into it).
// ---------------------------------------------------------------------------

template <typename T>
struct DevBuf {
  T *p = nullptr;
  explicit DevBuf(size_t count) { HIP_CHECK(hipMalloc(&p, count * sizeof(T))); }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
};

struct Event {
  hipEvent_t e = nullptr;
  Event() { HIP_CHECK(hipEventCreate(&e)); }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
};

constexpr int kProbeGrid = 2048;  // ≫256 workgroups: fills all 8 XCDs
constexpr int kCopyGrid = 4096;
constexpr int kBlock = 256;
constexpr uint64_t kProbeSeed = 0xA5A5F00DDEADBEEFull;
constexpr int kSentinelByte = 0xCD;
constexpr uint64_t kSentinelWord = 0xCDCDCDCDCDCDCDCDull;
constexpr long long kMaxWords = 1ll << 40;  // keeps every size_t product exact

int device_count() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return 0;
  return n;
}

// --- MFMA: operands, host reference, judge ---------------------------------

using Operands = std::pair<std::vector<float>, std::vector<float>>;

// The probe's first tile: asymmetric small dyadic operands (a symmetric B
// would mask a row/col swap).  Proves the lane mapping.
Operands stock_operands() {
  std::vector<float> A(16 * 4), B(4 * 16);
  for (int r = 0; r < 16; ++r)
    for (int k = 0; k < 4; ++k) A[r * 4 + k] = 0.25f * r - 1.5f * k + 0.125f;
  for (int k = 0; k < 4; ++k)
    for (int c = 0; c < 16; ++c) B[k * 16 + c] = 0.5f * k * k - 0.0625f * c + 1.f;
  return {A, B};
}

// A normal float with a full 24-bit significand from a fixed 64-bit LCG:
// random sign, exponent in [-8, 7], random 23 fraction bits.
float lcg_float(uint64_t &state) {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  uint32_t x = (uint32_t)(state >> 32);
  uint32_t bits = (x & 0x80000000u) | ((119u + ((x >> 23) & 15u)) << 23) |
                  (x & 0x007fffffu);
  float f;
  std::memcpy(&f, &bits, sizeof f);
  return f;
}

// The probe's second tile: operands that toggle every mantissa bit.  B is
// dense; row r of A is non-zero only at k = r % 4, so every output is ONE
// product plus zeros, C[r][c] = A[r][r%4]·B[r%4][c].  That is a single
// correct rounding whatever the unit's accumulation order and whether or
// not it fuses, so bitwise equality with the host chain is a contract, not
// an observation.  All four k-groups of A lanes and all 64 B lanes carry
// full-mantissa values.
Operands full_mantissa_operands() {
  std::vector<float> A(16 * 4, 0.f), B(4 * 16);
  uint64_t state = 0x243F6A8885A308D3ull;
  for (int r = 0; r < 16; ++r) A[r * 4 + (r % 4)] = lcg_float(state);
  for (int i = 0; i < 4 * 16; ++i) B[i] = lcg_float(state);
  return {A, B};
}

void require_tile(const std::vector<float> &A, const std::vector<float> &B) {
  if (A.size() != 16 * 4 || B.size() != 4 * 16)
    throw py::value_error("A must hold 16x4 and B 4x16 floats (64 each)");
}

// The host fmaf chain the probe judges against.
std::vector<float> mfma_reference(const std::vector<float> &A,
                                  const std::vector<float> &B) {
  require_tile(A, B);
  std::vector<float> ref(16 * 16, 0.f);
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 16; ++c)
      for (int k = 0; k < 4; ++k)
        ref[r * 16 + c] = fmaf(A[r * 4 + k], B[k * 16 + c], ref[r * 16 + c]);
  return ref;
}

// The probe's judge: exact-f32 contract, compared as bit patterns (so a NaN
// never equals a number and -0.0 is not +0.0).
int count_mismatches(const std::vector<float> &C, const std::vector<float> &ref) {
  if (C.size() != ref.size())
    throw py::value_error("C and ref differ in length");
  int bad = 0;
  for (size_t i = 0; i < C.size(); ++i) {
    uint32_t x, y;
    std::memcpy(&x, &C[i], sizeof x);
    std::memcpy(&y, &ref[i], sizeof y);
    if (x != y) ++bad;
  }
  return bad;
}

// One launch of mfma_canary_kernel on the current device.
std::vector<float> run_mfma(const std::vector<float> &A,
                            const std::vector<float> &B, float *launch_ms) {
  std::vector<float> C(16 * 16);
  DevBuf<float> dA(A.size()), dB(B.size()), dC(C.size());
  HIP_CHECK(hipMemcpy(dA.p, A.data(), A.size() * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dB.p, B.data(), B.size() * 4, hipMemcpyHostToDevice));
  // a kernel that wrote nothing must not be judged on stale memory
  HIP_CHECK(hipMemset(dC.p, 0xFF, C.size() * 4));
  Event t0, t1;
  HIP_CHECK(hipEventRecord(t0.e));
  mfma_canary_kernel<<<1, 64>>>(dA.p, dB.p, dC.p);
  HIP_CHECK(hipEventRecord(t1.e));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  if (launch_ms) HIP_CHECK(hipEventElapsedTime(launch_ms, t0.e, t1.e));
  HIP_CHECK(hipMemcpy(C.data(), dC.p, C.size() * 4, hipMemcpyDeviceToHost));
  return C;
}

std::vector<float> mfma_tile(int device, const std::vector<float> &A,
                             const std::vector<float> &B) {
  require_tile(A, B);
  HIP_CHECK(hipSetDevice(device));
  return run_mfma(A, B, nullptr);
}

// --- VRAM walk and copy ----------------------------------------------------

void require_launch(int grid, int block) {
  if (grid < 1 || grid > 65535 || block < 1 || block > 1024)
    throw py::value_error("grid must be in 1..65535 and block in 1..1024");
}

// vram_check_pattern over the first n words of buf, on the current device.
unsigned long long check_pattern(const uint64_t *buf, size_t n, uint64_t seed,
                                 int grid, int block) {
  DevBuf<unsigned long long> dbad(1);
  HIP_CHECK(hipMemset(dbad.p, 0, sizeof(unsigned long long)));
  vram_check_pattern<<<grid, block>>>(buf, n, seed, dbad.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  unsigned long long hbad = 0;
  HIP_CHECK(hipMemcpy(&hbad, dbad.p, sizeof(hbad), hipMemcpyDeviceToHost));
  return hbad;
}

// True when the `guard` words after buf[n] still hold the sentinel.
bool guard_intact(const uint64_t *buf, size_t n, size_t guard) {
  std::vector<uint64_t> g(guard);
  if (guard)
    HIP_CHECK(hipMemcpy(g.data(), buf + n, guard * sizeof(uint64_t),
                        hipMemcpyDeviceToHost));
  for (uint64_t w : g)
    if (w != kSentinelWord) return false;
  return true;
}

py::dict vram_walk(int device, long long n_words, uint64_t seed, int grid,
                   int block, long long guard_words,
                   const std::vector<std::pair<long long, uint64_t>> &corrupt,
                   bool dump) {
  if (n_words < 1 || n_words > kMaxWords)
    throw py::value_error("n_words must be at least 1: a walk over nothing "
                          "verifies nothing");
  if (guard_words < 0 || guard_words > kMaxWords)
    throw py::value_error("guard_words must not be negative");
  require_launch(grid, block);
  const size_t n = (size_t)n_words, total = n + (size_t)guard_words;
  for (const auto &c : corrupt)
    if (c.first < 0 || (size_t)c.first >= total)
      throw py::value_error("corrupt index outside the buffer");

  HIP_CHECK(hipSetDevice(device));
  DevBuf<uint64_t> buf(total);
  HIP_CHECK(hipMemset(buf.p, kSentinelByte, total * sizeof(uint64_t)));
  vram_write_pattern<<<grid, block>>>(buf.p, n, seed);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  for (const auto &c : corrupt) {
    uint64_t w = 0;
    HIP_CHECK(hipMemcpy(&w, buf.p + c.first, sizeof w, hipMemcpyDeviceToHost));
    w ^= c.second;
    HIP_CHECK(hipMemcpy(buf.p + c.first, &w, sizeof w, hipMemcpyHostToDevice));
  }
  py::dict out;
  out["mismatches"] = (py::int_)check_pattern(buf.p, n, seed, grid, block);
  out["guard_intact"] = guard_intact(buf.p, n, (size_t)guard_words);
  if (dump) {
    std::string raw(total * sizeof(uint64_t), '\0');
    HIP_CHECK(hipMemcpy(&raw[0], buf.p, raw.size(), hipMemcpyDeviceToHost));
    out["buffer"] = py::bytes(raw);
  }
  return out;
}

py::dict copy_walk(int device, long long n4, int grid, int block,
                   long long guard_words) {
  if (n4 < 1 || n4 > kMaxWords / 2)
    throw py::value_error("n4 must be at least 1: a copy of nothing verifies "
                          "nothing");
  if (guard_words < 0 || guard_words > kMaxWords)
    throw py::value_error("guard_words must not be negative");
  require_launch(grid, block);
  const size_t n = 2 * (size_t)n4, total = n + (size_t)guard_words;

  HIP_CHECK(hipSetDevice(device));
  DevBuf<uint64_t> src(n), dst(total);
  HIP_CHECK(hipMemset(dst.p, kSentinelByte, total * sizeof(uint64_t)));
  vram_write_pattern<<<kProbeGrid, kBlock>>>(src.p, n, kProbeSeed);
  bw_copy<<<grid, block>>>((const float4 *)src.p, (float4 *)dst.p, (size_t)n4);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  py::dict out;
  out["mismatches"] =
      (py::int_)check_pattern(dst.p, n, kProbeSeed, kProbeGrid, kBlock);
  out["guard_intact"] = guard_intact(dst.p, n, (size_t)guard_words);
  return out;
}

// --- the production probe --------------------------------------------------

py::dict probe(int device, int vram_probe_mb, bool bandwidth) {
  if (vram_probe_mb < 1)
    throw py::value_error("vram_probe_mb must be at least 1: a probe that "
                          "checks nothing must not report healthy");
  py::dict out;
  HIP_CHECK(hipSetDevice(device));

  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  out["arch"] = std::string(prop.gcnArchName);
  out["name"] = std::string(prop.name);
  out["vram_total_bytes"] = (py::int_)prop.totalGlobalMem;
  out["multi_processor_count"] = prop.multiProcessorCount;

  // --- 1+2: MFMA canary: stock tile (lane map), full-mantissa tile --------
  float launch_ms = 0;
  Operands stock = stock_operands(), full = full_mantissa_operands();
  int mfma_bad =
      count_mismatches(run_mfma(stock.first, stock.second, &launch_ms),
                       mfma_reference(stock.first, stock.second)) +
      count_mismatches(run_mfma(full.first, full.second, nullptr),
                       mfma_reference(full.first, full.second));
  out["mfma_ok"] = (mfma_bad == 0);
  out["mfma_mismatches"] = mfma_bad;
  out["mfma_launch_ms"] = launch_ms;

  // --- 3: VRAM pattern walk ------------------------------------------------
  size_t probe_bytes = (size_t)vram_probe_mb << 20;
  size_t n = probe_bytes / sizeof(uint64_t);
  DevBuf<uint64_t> buf(n);
  vram_write_pattern<<<kProbeGrid, kBlock>>>(buf.p, n, kProbeSeed);
  unsigned long long hbad = check_pattern(buf.p, n, kProbeSeed, kProbeGrid, kBlock);
  out["vram_ok"] = (hbad == 0);
  out["vram_mismatches"] = (py::int_)hbad;
  out["vram_probed_bytes"] = (py::int_)probe_bytes;

  // --- 4: optional HBM streaming bandwidth, copy verified -------------------
  unsigned long long copy_bad = 0;
  if (bandwidth) {
    size_t n4 = n / 2;  // reuse buf as src; dst is a second span
    DevBuf<uint64_t> dst(n);
    HIP_CHECK(hipMemset(dst.p, kSentinelByte, n * sizeof(uint64_t)));
    Event t0, t1;
    bw_copy<<<kCopyGrid, kBlock>>>((const float4 *)buf.p, (float4 *)dst.p, n4);  // warm
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipEventRecord(t0.e));
    bw_copy<<<kCopyGrid, kBlock>>>((const float4 *)buf.p, (float4 *)dst.p, n4);
    HIP_CHECK(hipEventRecord(t1.e));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, t0.e, t1.e));
    double gb = 2.0 * n4 * sizeof(float4) / 1e9;  // read + write
    out["hbm_copy_gbps"] = gb / (ms / 1e3);
    // dst must now carry buf's pattern word for word; the sentinel fill
    // turns a copy that stopped short into mismatches
    copy_bad = check_pattern(dst.p, n, kProbeSeed, kProbeGrid, kBlock);
    out["hbm_copy_mismatches"] = (py::int_)copy_bad;
  }

  out["ok"] = (mfma_bad == 0 && hbad == 0 && copy_bad == 0);
  return out;
}

}  // namespace

PYBIND11_MODULE(_canary, m) {
  m.doc() = "MI355X deep health probe (MFMA + VRAM canary kernels, gfx950)";
  m.def("device_count", &device_count);
  m.def("probe", &probe, py::arg("device") = 0, py::arg("vram_probe_mb") = 64,
        py::arg("bandwidth") = false);
  // host only
  m.def("stock_operands", &stock_operands);
  m.def("full_mantissa_operands", &full_mantissa_operands);
  m.def("mfma_reference", &mfma_reference, py::arg("A"), py::arg("B"));
  m.def("count_mismatches", &count_mismatches, py::arg("C"), py::arg("ref"));
  m.def("pattern_word",
        [](uint64_t i, uint64_t seed) { return pattern_at((size_t)i, seed); },
        py::arg("i"), py::arg("seed"));
  // one kernel each, on caller-supplied data
  m.def("mfma_tile", &mfma_tile, py::arg("device"), py::arg("A"), py::arg("B"));
  m.def("vram_walk", &vram_walk, py::arg("device"), py::arg("n_words"),
        py::arg("seed"), py::arg("grid") = kProbeGrid, py::arg("block") = kBlock,
        py::arg("guard_words") = 0,
        py::arg("corrupt") = std::vector<std::pair<long long, uint64_t>>{},
        py::arg("dump") = false);
  m.def("copy_walk", &copy_walk, py::arg("device"), py::arg("n4"),
        py::arg("grid") = kCopyGrid, py::arg("block") = kBlock,
        py::arg("guard_words") = 64);
}
