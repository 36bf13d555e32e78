// Profiling entry points (flow_profile_* in include/flow_hip.h): the event
// brackets around the in-solver SpMV of la_kernels.hip, the streaming kernels
// that measure what HBM sustains, the trace markers -- and the two host-side
// views of the CSR-stream tiling that tests and the row-block builder read.
#include "common.h"
#include "csr_stream.h"
#include "la_internal.h"

using namespace flow;

// nonzeros a CSR-stream row block of an operator of `kind` may hold (the host
// builds the row blocks: flow_amd/fem/space.py)
extern "C" int flow_spmv_tile_nnz(int kind) {
  return (kind == 2 || kind == 4) ? kTile2 - 2 : kTile - 2;
}

// the workgroup -> tile mapping of the CSR-stream kernels, for host-side tests
extern "C" int flow_xcd_tile_host(int block, int nblocks) {
  return xcd_tile(block, nblocks);
}

extern "C" int flow_profile_spmv_begin(int rows, int max_launches) {
  SpmvProfile& pf = g_spmv_profile;
  FLOW_REQUIRE(rows > 0 && max_launches > 0 && max_launches <= 100000,
               "profile arguments");
  FLOW_REQUIRE(pf.ev == nullptr, "a profile is already running");
  pf.ev = new hipEvent_t[2 * static_cast<size_t>(max_launches)];
  for (int i = 0; i < 2 * max_launches; ++i)
    FLOW_CHECK_HIP(hipEventCreate(&pf.ev[i]));
  pf.rows = rows;
  pf.used = 0;
  pf.cap = max_launches;
  return FLOW_OK;
}

__global__ void profile_null_kernel() {}

// keeps the chip busy for ~20 us (constant 100 MHz counter; bounded loop), so
// that the launch behind it is dispatched while it runs -- as inside a solver
__global__ void profile_busy_kernel() {
  const unsigned long long t0 = wall_clock64();
  for (int i = 0; i < 100000; ++i) {
    if (wall_clock64() - t0 > 2000ull) break;
    __builtin_amdgcn_s_sleep(8);
  }
}

// What an event pair measures around NOTHING: the dispatch latency that every
// bracketed launch above includes on top of the kernel's own execution time
// (rocprofv3's kernel duration does not).  Median of 33 null launches, each
// behind a kernel that is still running when it is enqueued, microseconds.
extern "C" int flow_profile_event_overhead(double* overhead_us, void* stream) {
  FLOW_REQUIRE(overhead_us != nullptr, "overhead result");
  hipStream_t st = as_stream(stream);
  constexpr int kN = 33;
  hipEvent_t ev[2 * kN];
  for (int i = 0; i < 2 * kN; ++i) FLOW_CHECK_HIP(hipEventCreate(&ev[i]));
  for (int i = 0; i < kN; ++i) {
    // (a running kernel in front, as in the solver: the stream is never idle
    // and the bracketed launch is dispatched while its predecessor executes)
    hipLaunchKernelGGL(profile_busy_kernel, dim3(256), dim3(64), 0, st);
    FLOW_CHECK_HIP(hipEventRecord(ev[2 * i], st));
    hipLaunchKernelGGL(profile_null_kernel, dim3(1), dim3(64), 0, st);
    FLOW_CHECK_HIP(hipEventRecord(ev[2 * i + 1], st));
  }
  FLOW_CHECK_HIP(hipStreamSynchronize(st));
  double t[kN];
  for (int i = 0; i < kN; ++i) {
    float ms = 0.0f;
    FLOW_CHECK_HIP(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
    t[i] = 1.0e3 * ms;
  }
  for (int i = 0; i < 2 * kN; ++i) (void)hipEventDestroy(ev[i]);
  for (int i = 1; i < kN; ++i)          // insertion sort, median
    for (int j = i; j > 0 && t[j] < t[j - 1]; --j) {
      const double tmp = t[j];
      t[j] = t[j - 1];
      t[j - 1] = tmp;
    }
  *overhead_us = t[kN / 2];
  return FLOW_OK;
}

extern "C" int flow_profile_spmv_end(double* total_us, int* launches) {
  SpmvProfile& pf = g_spmv_profile;
  FLOW_REQUIRE(total_us && launches, "profile results");
  FLOW_REQUIRE(pf.ev != nullptr, "no profile is running");
  double total = 0.0;
  int rc = FLOW_OK;
  for (int i = 0; i < pf.used && rc == FLOW_OK; ++i) {
    float ms = 0.0f;
    if (hipEventSynchronize(pf.ev[2 * i + 1]) != hipSuccess ||
        hipEventElapsedTime(&ms, pf.ev[2 * i], pf.ev[2 * i + 1]) != hipSuccess) {
      set_error("reading the SpMV profile events failed");
      rc = FLOW_HIP_ERROR;
    }
    total += 1.0e3 * ms;
  }
  for (int i = 0; i < 2 * pf.cap; ++i) (void)hipEventDestroy(pf.ev[i]);
  delete[] pf.ev;
  *total_us = total;
  *launches = pf.used;
  pf = SpmvProfile();
  return rc;
}

// plain streaming kernels, 16 bytes per lane and load: what this chip's HBM
// sustains for the simplest possible kernels (bench.py times them with HIP
// events and quotes the roofline kernel against them as well as against the
// 8 TB/s of the data sheet).  Variants were timed on the box
// (tools/micro/copy_ceiling.hip): copy with non-temporal loads and stores, four
// per lane in flight, 8192 workgroups: 5.17 TB/s (plain: 4.6-4.85); read-only,
// eight loads in flight, 16384 workgroups: 5.85 TB/s.
__global__ __launch_bounds__(kBlock) void stream_copy_kernel(
    size_t n2, const double2* __restrict__ src, double2* __restrict__ dst) {
  constexpr int U = 4;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  for (; i + (U - 1) * stride < n2; i += U * stride) {
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u].x = __builtin_nontemporal_load(&src[i + u * stride].x);
      v[u].y = __builtin_nontemporal_load(&src[i + u * stride].y);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      __builtin_nontemporal_store(v[u].x, &dst[i + u * stride].x);
      __builtin_nontemporal_store(v[u].y, &dst[i + u * stride].y);
    }
  }
  for (; i < n2; i += stride) dst[i] = src[i];
}

__global__ __launch_bounds__(kBlock) void stream_read_kernel(
    size_t n2, const double2* __restrict__ src, double* __restrict__ sink) {
  constexpr int U = 8;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  double acc = 0.0;
  for (; i + (U - 1) * stride < n2; i += U * stride) {
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = src[i + u * stride];
#pragma unroll
    for (int u = 0; u < U; ++u) acc += v[u].x + v[u].y;
  }
  for (; i < n2; i += stride) acc += src[i].x + src[i].y;
  // (never true for the buffers bench.py passes; keeps the loads alive)
  if (acc == 12345.678) sink[0] = acc;
}

extern "C" int flow_profile_stream_copy(size_t n, const double* src, double* dst,
                                        void* stream) {
  FLOW_REQUIRE(n >= 2 && n % 2 == 0 && src != nullptr, "stream copy arguments");
  FLOW_REQUIRE(reinterpret_cast<uintptr_t>(src) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(dst) % 16 == 0 && dst != nullptr,
               "stream copy: 16-byte aligned buffers");
  hipLaunchKernelGGL(stream_copy_kernel, dim3(8192), dim3(kBlock), 0,
                     as_stream(stream), n / 2,
                     reinterpret_cast<const double2*>(src),
                     reinterpret_cast<double2*>(dst));
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_profile_stream_read(size_t n, const double* src, double* sink,
                                        void* stream) {
  FLOW_REQUIRE(n >= 2 && n % 2 == 0 && src != nullptr && sink != nullptr,
               "stream read arguments");
  FLOW_REQUIRE(reinterpret_cast<uintptr_t>(src) % 16 == 0,
               "stream read: 16-byte aligned buffer");
  hipLaunchKernelGGL(stream_read_kernel, dim3(16384), dim3(kBlock), 0,
                     as_stream(stream), n / 2,
                     reinterpret_cast<const double2*>(src), sink);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// an empty kernel whose GRID SIZE is the marker id: profiles/summarize.py finds
// the timed window of bench.py in a rocprofv3 kernel trace by these launches
__global__ void profile_marker_kernel() {}

extern "C" int flow_profile_marker(int id, void* stream) {
  FLOW_REQUIRE(id >= 1 && id <= 1024, "marker id");
  hipLaunchKernelGGL(profile_marker_kernel, dim3(id), dim3(64), 0,
                     as_stream(stream));
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
