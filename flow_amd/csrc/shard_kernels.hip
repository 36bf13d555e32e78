// K15: domain decomposition over the GPUs of one node (include/flow_hip.h).
// One communication primitive -- comm->allreduce: sum of the head of comm->buf
// over the ranks -- carries the dot products, the partial coarse residuals AND
// the halos (own slots filled, all others zero: the sum is the concatenation).
// The sharded CG and GMRES run the kernels of la_kernels.hip and
// krylov_kernels.hip on a rank's rows (declarations: la_internal.h).
#include <cstring>

#include "common.h"
#include "la_internal.h"

using namespace flow;

// ---- flow_peer: the blocks and their IPC handles ---------------------------
extern "C" int flow_peer_alloc(int land_cap, void** base_out, char* handle_out) {
  FLOW_REQUIRE(land_cap > 0 && base_out && handle_out, "flow_peer_alloc arguments");
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
  const size_t bytes = sizeof(unsigned long long) * FLOW_PEER_FLAGS +
                       2 * sizeof(double) * static_cast<size_t>(land_cap);
  void* base = nullptr;
  // fine-grained where the runtime grants it (flag words polled across GPUs);
  // plain device memory otherwise -- all flag and landing traffic is system
  // scope either way
  if (hipExtMallocWithFlags(&base, bytes, hipDeviceMallocFinegrained) != hipSuccess) {
    (void)hipGetLastError();
    FLOW_CHECK_HIP(hipMalloc(&base, bytes));
  }
  FLOW_CHECK_HIP(hipMemset(base, 0, bytes));
  FLOW_CHECK_HIP(hipDeviceSynchronize());
  hipIpcMemHandle_t h;
  hipError_t err = hipIpcGetMemHandle(&h, base);
  if (err != hipSuccess) {
    // (some runtimes refuse to export fine-grained memory: plain memory then)
    (void)hipGetLastError();
    (void)hipFree(base);
    FLOW_CHECK_HIP(hipMalloc(&base, bytes));
    FLOW_CHECK_HIP(hipMemset(base, 0, bytes));
    FLOW_CHECK_HIP(hipDeviceSynchronize());
    FLOW_CHECK_HIP(hipIpcGetMemHandle(&h, base));
  }
  memcpy(handle_out, &h, sizeof(h));
  *base_out = base;
  return FLOW_OK;
}

extern "C" int flow_peer_open(const char* handle, void** base_out) {
  FLOW_REQUIRE(handle && base_out, "flow_peer_open arguments");
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof(h));
  FLOW_CHECK_HIP(hipIpcOpenMemHandle(base_out, h, hipIpcMemLazyEnablePeerAccess));
  return FLOW_OK;
}

extern "C" int flow_peer_close(void* mapped_base) {
  FLOW_REQUIRE(mapped_base != nullptr, "flow_peer_close argument");
  FLOW_CHECK_HIP(hipIpcCloseMemHandle(mapped_base));
  return FLOW_OK;
}

extern "C" int flow_peer_free(void* base) {
  FLOW_REQUIRE(base != nullptr, "flow_peer_free argument");
  FLOW_CHECK_HIP(hipFree(base));
  return FLOW_OK;
}

extern "C" int flow_peer_status(const flow_peer* peer,
                                unsigned long long* error_host, void* stream) {
  FLOW_REQUIRE(peer && peer->flags && error_host, "flow_peer_status arguments");
  hipStream_t st = as_stream(stream);
  FLOW_CHECK_HIP(hipMemcpyAsync(error_host, peer->flags + 4, sizeof(*error_host),
                                hipMemcpyDeviceToHost, st));
  FLOW_CHECK_HIP(hipStreamSynchronize(st));
  return FLOW_OK;
}

// sharded GMRES (outside the namespace, like the GMRES kernels of
// krylov_kernels.hip): block b sums the partials of value b (< nd: w.V_b ;
// nd: w.w ; nd+1: |V_j|^2) straight into the exchange buffer
__global__ __launch_bounds__(kBlock) void gmres_finish_kernel(
    int nparts, int nd, const double* __restrict__ partial,
    volatile double* __restrict__ mailbox) {
  const int b = blockIdx.x;
  const int v = b < nd ? b : kGmresMax + (b - nd);
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kBlock)
    s += load_scalar(partial + v * kRedBlocks + i);
  s = block_sum(s);
  if (threadIdx.x == 0) {
    mailbox[b] = s;
    __threadfence_system();
  }
}

namespace flow {

int check_comm(const flow_comm* c, long long need) {
  FLOW_REQUIRE(c != nullptr && c->allreduce != nullptr && c->buf != nullptr,
               "communicator");
  FLOW_REQUIRE(c->world >= 1 && c->world <= kNumSlots && c->rank >= 0 &&
                   c->rank < c->world,
               "communicator rank / world (at most 16 ranks)");
  FLOW_REQUIRE(c->capacity >= need, "exchange buffer too small");
  FLOW_REQUIRE(reinterpret_cast<uintptr_t>(c->buf) % 16 == 0,
               "exchange buffer must be 16-byte aligned");
  return FLOW_OK;
}

int check_rows(const flow_rows* R) {
  FLOW_REQUIRE(R != nullptr, "row ranges are NULL");
  FLOW_REQUIRE(0 <= R->e0 && R->e0 <= R->r0 && R->r0 < R->r1 && R->r1 <= R->e1 &&
                   R->e1 <= R->n,
               "row ranges");
  FLOW_REQUIRE(R->nhalo >= 0, "halo size");
  for (int i = 0; i < 2; ++i) {
    FLOW_REQUIRE(R->send_len[i] >= 0 && R->recv_len[i] >= 0, "halo lengths");
    FLOW_REQUIRE(R->send_len[i] == 0 ||
                     (R->send_row[i] >= R->r0 &&
                      R->send_row[i] + R->send_len[i] <= R->r1 &&
                      R->send_slot[i] >= 0 &&
                      R->send_slot[i] + R->send_len[i] <= R->nhalo),
                 "halo send range");
    FLOW_REQUIRE(R->recv_len[i] == 0 ||
                     (R->recv_row[i] >= R->e0 &&
                      R->recv_row[i] + R->recv_len[i] <= R->e1 &&
                      (R->recv_row[i] + R->recv_len[i] <= R->r0 ||
                       R->recv_row[i] >= R->r1) &&
                      R->recv_slot[i] >= 0 &&
                      R->recv_slot[i] + R->recv_len[i] <= R->nhalo),
                 "halo receive range");
  }
  return FLOW_OK;
}

int exchange(const flow_comm* c, int count) {
  const int rc = c->allreduce(c->user, count);
  if (rc != 0) {
    set_error("the all-reduce callback failed (code %d, %d doubles)", rc, count);
    return FLOW_HIP_ERROR;
  }
  return FLOW_OK;
}

// ---- halos from neighbour to neighbour (flow_peer) --------------------------
// Every rank owns a LANDING area its two neighbours have mapped (hipIpc): two
// buffers of land_cap doubles (exchange seq uses buffer seq & 1) and a block of
// 64-bit flags.  One exchange = one push and one pull launch around whatever is
// really summed:
//   push  a workgroup per side: wait until that neighbour has pulled exchange
//         seq - 2 (the landing buffer of this parity is free again: its
//         `consumed` word in MY block), copy my send slots of the packed
//         buffer into ITS landing buffer -- same slot numbering on all ranks --,
//         fence, then write seq into its `arrived` word;
//   pull  a workgroup per side: wait for my `arrived` word of that side, copy
//         the landing buffer's receive slots into my packed buffer (where the
//         unpack kernels look, as after an all-reduce), then write seq into the
//         neighbour's `consumed` word.
// Waits are bounded (spin_limit polls with a sleep in between): a neighbour
// that never arrives sets the error word of this rank's block and the kernel
// goes on -- nothing can hang the device; the host reads the word
// (flow_peer_status) behind its next read-back.  All flag traffic is system
// scope (past L2: the words live in another process, on another GPU).
constexpr int kPeerBlock = 256;
enum PeerFlag { kArrived = 0, kConsumed = 2, kPeerError = 4, kPeerFlags = 16 };

__device__ __forceinline__ unsigned long long peer_load(const unsigned long long* p) {
  return __hip_atomic_load(const_cast<unsigned long long*>(p), __ATOMIC_ACQUIRE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void peer_store(unsigned long long* p,
                                           unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// thread 0 waits for *flag >= want; false on time-out (error word set)
__device__ __forceinline__ bool peer_wait(const unsigned long long* flag,
                                          unsigned long long want, int limit,
                                          unsigned long long* err,
                                          unsigned long long code) {
  for (int it = 0; it < limit; ++it) {
    if (peer_load(flag) >= want) return true;
    __builtin_amdgcn_s_sleep(32);
  }
  peer_store(err, code);
  return false;
}

// free0 / free1: the exchange in which this rank LAST pushed into the same
// landing buffer of its left / right neighbour (0: never) -- that one must
// have been pulled before the buffer is written again
__global__ __launch_bounds__(kPeerBlock) void peer_push_kernel(
    flow_rows R, int ncomp, flow_peer P, unsigned long long seq,
    unsigned long long free0, unsigned long long free1,
    const double* __restrict__ packed) {
  const int sd = blockIdx.x;
  if (R.send_len[sd] <= 0 || P.nb_land[sd] == nullptr) return;
  const unsigned long long need = sd == 0 ? free0 : free1;
  if (threadIdx.x == 0 && need > 0)
    peer_wait(P.flags + kConsumed + sd, need, P.spin_limit, P.flags + kPeerError,
              (seq << 8) | (1 + sd));
  __syncthreads();
  double* land = P.nb_land[sd] + static_cast<size_t>(seq & 1) * P.land_cap;
  const int len = R.send_len[sd];
  for (int t = threadIdx.x; t < ncomp * len; t += kPeerBlock) {
    const int a = t / len, j = t - a * len;
    const size_t k = static_cast<size_t>(a) * R.nhalo + R.send_slot[sd] + j;
    __hip_atomic_store(land + k, packed[k], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __threadfence_system();
  __syncthreads();
  // I am this neighbour's neighbour on its OTHER side
  if (threadIdx.x == 0) peer_store(P.nb_flags[sd] + kArrived + (1 - sd), seq);
}

__global__ __launch_bounds__(kPeerBlock) void peer_pull_kernel(
    flow_rows R, int ncomp, flow_peer P, unsigned long long seq,
    double* __restrict__ packed) {
  const int sd = blockIdx.x;
  if (R.recv_len[sd] <= 0 || P.nb_flags[sd] == nullptr) return;
  if (threadIdx.x == 0)
    peer_wait(P.flags + kArrived + sd, seq, P.spin_limit, P.flags + kPeerError,
              (seq << 8) | (3 + sd));
  __syncthreads();
  const double* land = P.land + static_cast<size_t>(seq & 1) * P.land_cap;
  const int len = R.recv_len[sd];
  for (int t = threadIdx.x; t < ncomp * len; t += kPeerBlock) {
    const int a = t / len, j = t - a * len;
    const size_t k = static_cast<size_t>(a) * R.nhalo + R.recv_slot[sd] + j;
    packed[k] = __hip_atomic_load(const_cast<double*>(land + k), __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __syncthreads();
  if (threadIdx.x == 0) peer_store(P.nb_flags[sd] + kConsumed + (1 - sd), seq);
}

// One exchange of a packed buffer [sums (sum_count doubles) | ... | halo slots
// at hoff]: the sums through the all-reduce, the halo either with them (the
// whole buffer is summed: every rank wrote zeros into the others' slots) or,
// with a flow_peer, from neighbour to neighbour -- then only the first
// sum_count doubles are a collective, and none at all for a pure halo.
int exchange_halo(const flow_comm* C, const flow_rows* R, int ncomp, int sum_count,
                  int hoff, hipStream_t st) {
  const int nh = ncomp * R->nhalo;
  const flow_peer* P = C->peer;
  // (a halo larger than the landing buffers -- the slot numbering spans ALL
  // ranks' slots -- travels in the all-reduce like without a flow_peer: nh is
  // the same on every rank, so is this decision)
  if (P == nullptr || C->world == 1 || nh == 0 || nh > P->land_cap)
    return (hoff + nh > 0) ? exchange(C, hoff + nh) : FLOW_OK;
  FLOW_REQUIRE(P->flags && P->land && P->seq_host, "flow_peer pointers");
  // seq_host[0]: the exchange counter; seq_host[1 + 2 sd + parity]: my last
  // push into that landing buffer of neighbour sd (what it must have pulled
  // before this one may overwrite it -- not simply "two exchanges ago": an
  // exchange of a space that sends nothing to a side skips that side)
  unsigned long long* H = P->seq_host;
  const unsigned long long seq = ++H[0];
  const int par = static_cast<int>(seq & 1);
  const unsigned long long free0 = H[1 + par], free1 = H[3 + par];
  hipLaunchKernelGGL(peer_push_kernel, dim3(2), dim3(kPeerBlock), 0, st, *R, ncomp,
                     *P, seq, free0, free1, C->buf + hoff);
  for (int sd = 0; sd < 2; ++sd)
    if (R->send_len[sd] > 0 && P->nb_land[sd] != nullptr) H[1 + 2 * sd + par] = seq;
  FLOW_CHECK_LAUNCH();
  if (sum_count > 0) {
    int rc = exchange(C, sum_count);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(peer_pull_kernel, dim3(2), dim3(kPeerBlock), 0, st, *R, ncomp,
                     *P, seq, C->buf + hoff);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// halo[a*nhalo + k] <- the own boundary entries of x (global row index,
// component stride `stride`), zero in everybody else's slots
__global__ void shard_pack_kernel(flow_rows R, int ncomp,
                                  const double* __restrict__ x, int stride,
                                  double* __restrict__ halo) {
  const int total = ncomp * R.nhalo;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += gridDim.x * blockDim.x) {
    const int a = t / R.nhalo, k = t - a * R.nhalo;
    const double* xa = x + static_cast<size_t>(a) * stride;
    double v = 0.0;
#pragma unroll
    for (int sd = 0; sd < 2; ++sd)
      if (k >= R.send_slot[sd] && k < R.send_slot[sd] + R.send_len[sd])
        v = xa[R.send_row[sd] + (k - R.send_slot[sd])];
    halo[t] = v;
  }
}

// ghost rows of x <- the neighbours' slots of the summed buffer
__global__ void shard_unpack_kernel(flow_rows R, int ncomp,
                                    const double* __restrict__ halo,
                                    double* __restrict__ x, int stride) {
  const int per = R.recv_len[0] + R.recv_len[1];
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < ncomp * per;
       t += gridDim.x * blockDim.x) {
    const int a = t / per, k = t - a * per;
    const int sd = k < R.recv_len[0] ? 0 : 1;
    const int j = sd == 0 ? k : k - R.recv_len[0];
    x[static_cast<size_t>(a) * stride + R.recv_row[sd] + j] =
        load_scalar(halo + static_cast<size_t>(a) * R.nhalo + R.recv_slot[sd] + j);
  }
}

// x: indexed by global row (x[a*stride + row]); the halo travels at buf + off
static int halo(const flow_comm* C, const flow_rows* R, int ncomp, double* x,
                int stride, hipStream_t st) {
  const int count = ncomp * R->nhalo;
  if (count == 0) return FLOW_OK;      // a single rank
  hipLaunchKernelGGL(shard_pack_kernel, dim3(grid_for(count)), dim3(kBlock), 0,
                     st, *R, ncomp, x, stride, C->buf);
  FLOW_CHECK_LAUNCH();
  // (a pure halo: no sums -- with a flow_peer no collective at all)
  int rc = exchange_halo(C, R, ncomp, 0, 0, st);
  if (rc) return rc;
  const int per = R->recv_len[0] + R->recv_len[1];
  if (per > 0) {
    hipLaunchKernelGGL(shard_unpack_kernel, dim3(grid_for(ncomp * per)),
                       dim3(kBlock), 0, st, *R, ncomp, C->buf, x, stride);
    FLOW_CHECK_LAUNCH();
  }
  return FLOW_OK;
}

// ext-compact <- global-length field (ncomp components), and the ownership mask
__global__ void shard_compress_kernel(int ncomp, int me, int e0, int n,
                                      const double* __restrict__ src,
                                      double* __restrict__ dst) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < ncomp * me;
       t += gridDim.x * blockDim.x) {
    const int a = t / me, i = t - a * me;
    dst[t] = src[static_cast<size_t>(a) * n + e0 + i];
  }
}

__global__ void shard_expand_kernel(int ncomp, int me, int e0, int n,
                                    const double* __restrict__ src,
                                    double* __restrict__ dst) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < ncomp * me;
       t += gridDim.x * blockDim.x) {
    const int a = t / me, i = t - a * me;
    dst[static_cast<size_t>(a) * n + e0 + i] = src[t];
  }
}

__global__ void shard_own_kernel(int ncomp, int me, int lo, int hi,
                                 double* __restrict__ own) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < ncomp * me;
       t += gridDim.x * blockDim.x) {
    const int i = t % me;
    own[t] = (i >= lo && i < hi) ? 1.0 : 0.0;
  }
}

// dst (owned-compact, stride mo, ncomp comps) <-> src (other layout): generic
// strided 2-D copy  dst[a*ds + i] = src[a*ss + i], i < m
__global__ void shard_copy2d_kernel(int ncomp, int m, const double* __restrict__ src,
                                    int ss, double* __restrict__ dst, int ds,
                                    double scale, int accumulate) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < ncomp * m;
       t += gridDim.x * blockDim.x) {
    const int a = t / m, i = t - a * m;
    const double v = scale * src[static_cast<size_t>(a) * ss + i];
    double* d = dst + static_cast<size_t>(a) * ds + i;
    *d = accumulate ? *d + v : v;
  }
}

static int copy2d(int ncomp, int m, const double* src, int ss, double* dst,
                  int ds, hipStream_t st, double scale = 1.0,
                  int accumulate = 0) {
  hipLaunchKernelGGL(shard_copy2d_kernel, dim3(grid_for(ncomp * m)), dim3(kBlock),
                     0, st, ncomp, m, src, ss, dst, ds, scale, accumulate);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// buf[k] = (k == rank) ? max(v[0..nv)) : 0, k < world
__global__ void shard_rank_slot_kernel(int world, int rank, int nv,
                                       const double* __restrict__ v,
                                       double* __restrict__ buf) {
  const int k = threadIdx.x;
  if (k >= world) return;
  double m = 0.0;
  if (k == rank)
    for (int i = 0; i < nv; ++i) m = fmax(m, load_scalar(v + i));
  buf[k] = m;
}

// ---------------------------------------------------------------------------
// sharded CG (Jacobi or multigrid V-cycle), ext-compact vectors
// ---------------------------------------------------------------------------
// block 0: the three partial lists -> buf[0..2], buf[3] = *extra (or 0);
// blocks >= 1: halo slots of w at buf + 4 (own boundary entries, else 0)
__global__ __launch_bounds__(kScalarBlock) void shard_finish_pack_kernel(
    flow_rows R, int ncomp, int np, int nd, const double* __restrict__ gpart,
    const double* __restrict__ rpart, const double* __restrict__ dpart,
    const double* __restrict__ extra, const double* __restrict__ w, int stride,
    double* __restrict__ buf, const double* __restrict__ stop, int hoff = 4) {
  if (stopped(stop)) return;
  if (blockIdx.x > 0) {
    const int total = ncomp * R.nhalo;
    double* halo = buf + hoff;
    for (int t = (blockIdx.x - 1) * blockDim.x + threadIdx.x; t < total;
         t += (gridDim.x - 1) * blockDim.x) {
      const int a = t / R.nhalo, k = t - a * R.nhalo;
      const double* wa = w + static_cast<size_t>(a) * stride;
      double v = 0.0;
#pragma unroll
      for (int sd = 0; sd < 2; ++sd)
        if (k >= R.send_slot[sd] && k < R.send_slot[sd] + R.send_len[sd])
          v = wa[R.send_row[sd] + (k - R.send_slot[sd])];
      halo[t] = v;
    }
    return;
  }
  __shared__ double wsum[3][kScalarBlock / 64];
  double g = 0.0, rr = 0.0, d = 0.0;
  for (int i = threadIdx.x; i < np; i += kScalarBlock) {
    g += load_scalar(gpart + i);
    rr += load_scalar(rpart + i);
  }
  for (int i = threadIdx.x; i < nd; i += kScalarBlock) d += load_scalar(dpart + i);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    g += __shfl_down(g, off, 64);
    d += __shfl_down(d, off, 64);
    rr += __shfl_down(rr, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    wsum[0][threadIdx.x >> 6] = g;
    wsum[1][threadIdx.x >> 6] = d;
    wsum[2][threadIdx.x >> 6] = rr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    g = d = rr = 0.0;
    for (int k = 0; k < kScalarBlock / 64; ++k) {
      g += wsum[0][k];
      d += wsum[1][k];
      rr += wsum[2][k];
    }
    buf[0] = g;
    buf[1] = d;
    buf[2] = rr;
    buf[3] = extra ? load_scalar(extra) : 0.0;
  }
}

// thread 0 of block 0: Chronopoulos-Gear scalars + the stopping test from the
// summed buf[0..3] (first: the target from buf[3] = |B b|^2), exactly as
// cg_scalar_kernel; everybody: ghost rows of w <- the neighbours' slots
// ncopy > 0: also copy_dst[0, ncopy) <- buf[copy_off, +ncopy) (the summed
// coarse image C w of the two-collective multigrid CG)
__global__ void shard_scalar_unpack_kernel(flow_rows R, int ncomp, int first,
                                           double rtol2, double atol2,
                                           const double* __restrict__ buf,
                                           double* __restrict__ S,
                                           double* __restrict__ w, int stride,
                                           int ncopy = 0, int copy_off = 0,
                                           double* __restrict__ copy_dst = nullptr,
                                           int hoff = 4) {
  if (stopped(S + kDone)) return;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < ncopy;
       t += gridDim.x * blockDim.x)
    copy_dst[t] = load_scalar(buf + copy_off + t);
  const int per = R.recv_len[0] + R.recv_len[1];
  const double* halo = buf + hoff;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < ncomp * per;
       t += gridDim.x * blockDim.x) {
    const int a = t / per, k = t - a * per;
    const int sd = k < R.recv_len[0] ? 0 : 1;
    const int j = sd == 0 ? k : k - R.recv_len[0];
    w[static_cast<size_t>(a) * stride + R.recv_row[sd] + j] =
        load_scalar(halo + static_cast<size_t>(a) * R.nhalo + R.recv_slot[sd] + j);
  }
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double g = load_scalar(buf), d = load_scalar(buf + 1),
               rr = load_scalar(buf + 2);
  double alpha, beta;
  if (first) {
    beta = 0.0;
    alpha = (d != 0.0) ? g / d : 0.0;
    store_scalar(S + kB2, load_scalar(buf + 3));
    store_scalar(S + kTarget2, fmax(rtol2 * load_scalar(buf + 3), atol2));
    store_scalar(S + kIter, 0.0);
    // first == 2: the guarded start of cg_scalar_kernel -- the sums are the
    // same on every rank, so is the verdict
    if (first == 2 && rr > load_scalar(buf + 3)) {
      store_scalar(S + kConvIt, 0.0);
      store_scalar(S + kRes2, rr);
      store_scalar(S + kDone, 5.0);
      return;
    }
  } else {
    const double g_old = load_scalar(S + kGamma);
    const double a_old = load_scalar(S + kAlpha);
    beta = (g_old != 0.0) ? g / g_old : 0.0;
    const double den = (a_old != 0.0) ? d - beta * g / a_old : 0.0;
    alpha = (den != 0.0) ? g / den : 0.0;
  }
  const double k = first ? 0.0 : load_scalar(S + kIter);
  const double target2 =
      first ? fmax(rtol2 * load_scalar(buf + 3), atol2) : load_scalar(S + kTarget2);
  const bool nan = !(rr == rr);
  if (nan || rr <= target2) {
    store_scalar(S + kConvIt, k);
    store_scalar(S + kDone, nan ? 2.0 : 1.0);
    alpha = beta = 0.0;
  }
  store_scalar(S + kIter, k + 1.0);
  store_scalar(S + kGamma, g);
  store_scalar(S + kAlpha, alpha);
  store_scalar(S + kBeta, beta);
  store_scalar(S + kRes2, rr);
}

// masked dots of ext-compact vectors: sum own*a0*b0 [, own*a1*b1]
__global__ __launch_bounds__(kBlock) void shard_dot2_kernel(
    int n, const double* __restrict__ own, const double* __restrict__ a0,
    const double* __restrict__ b0, const double* __restrict__ a1,
    const double* __restrict__ b1, double* __restrict__ p0,
    double* __restrict__ p1) {
  double s0 = 0.0, s1 = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    if (own[i] != 0.0) {      // select, not multiply: ghost entries may be NaN
      s0 += a0[i] * b0[i];
      s1 += a1[i] * b1[i];
    }
  }
  s0 = block_sum(s0);
  s1 = block_sum(s1);
  if (threadIdx.x == 0) {
    p0[blockIdx.x] = s0;
    p1[blockIdx.x] = s1;
  }
}

struct ShardCg {
  const flow_comm* C;
  const flow_rows* R;
  const flow_operator* A;
  const flow_mg_shard* G;     // nullptr: Jacobi
  int ncomp, me, m, L;
  double *partial, *S, *r, *z, *w, *p, *s, *xc, *bc, *dc, *own, *t;
  double *dpart, *mpart;
  hipStream_t st;
  template <class T>
  T* sh(T* v) const { return v - R->e0; }   // index by global row
};

// the coarse image of CG's recurrences (two-collective form):
//   rc_s = rc_w + beta rc_s ;  rc_r -= alpha rc_s
__global__ void shard_rc_update_kernel(int n1, const double* __restrict__ S,
                                       const double* __restrict__ rc_w,
                                       double* __restrict__ rc_s,
                                       double* __restrict__ rc_r) {
  if (stopped(S + kDone)) return;
  const double alpha = load_scalar(S + kAlpha);
  const double beta = load_scalar(S + kBeta);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n1;
       i += gridDim.x * blockDim.x) {
    const double si = rc_w[i] + beta * rc_s[i];
    rc_s[i] = si;
    rc_r[i] -= alpha * si;
  }
}

// iterations between two recomputations of the coarse images (see shard_cg)
constexpr int kRcRefresh = 8;
__global__ void shard_rc_refresh_kernel(int n1, const double* __restrict__ buf,
                                        double* __restrict__ rc_r,
                                        double* __restrict__ rc_s,
                                        const double* __restrict__ stop) {
  if (stopped(stop)) return;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n1;
       i += gridDim.x * blockDim.x) {
    rc_r[i] = load_scalar(buf + i);
    rc_s[i] = load_scalar(buf + n1 + i);
  }
}

static inline bool shard_two_launch(const flow_mg_shard* G) {
  return G && G->Cg.rowptr != nullptr && G->mg->C[0].rowptr != nullptr;
}

// the up-sweep of level 0 on the owned rows from the coarse solution M->x[1]
static int shard_up0(const ShardCg& c, const double* r, double* z, double* gpart,
                     double* rpart, int* nparts, const double* stop) {
  const flow_mg* M = c.G->mg;
  const flow_operator* A0 = &c.G->Ah0;
  const flow_operator* P0 = &c.G->Ps0;
  double* const none = nullptr;
  if (shard_two_launch(c.G)) {
    const dim3 grid(c.G->up_nblocks0);
    if (gpart)
      hipLaunchKernelGGL(mg_up2_kernel<true>, grid, dim3(kBlock), 0, c.st,
                         c.G->up_rowblocks0, P0->rowptr, P0->cols, P0->vals[0],
                         A0->rowptr, A0->cols, A0->vals[0], M->x[1], c.sh(r),
                         M->dinv[0], M->omega, c.sh(z), gpart, rpart, stop,
                         c.R->r0, c.R->r1);
    else
      hipLaunchKernelGGL(mg_up2_kernel<false>, grid, dim3(kBlock), 0, c.st,
                         c.G->up_rowblocks0, P0->rowptr, P0->cols, P0->vals[0],
                         A0->rowptr, A0->cols, A0->vals[0], M->x[1], c.sh(r),
                         M->dinv[0], M->omega, c.sh(z), none, none, stop);
    if (gpart) *nparts = c.G->up_nblocks0;
  } else if (gpart) {
    hipLaunchKernelGGL((mg_level_kernel<1, true>), dim3(P0->nblocks), dim3(kBlock),
                       0, c.st, P0->rowptr, P0->cols, P0->vals[0], P0->rowblocks,
                       M->x[1], c.sh(r), c.sh(c.t), M->dinv[0], M->omega, c.sh(z),
                       gpart, rpart, stop);
    *nparts = P0->nblocks;
  } else {
    hipLaunchKernelGGL((mg_level_kernel<1, false>), dim3(P0->nblocks),
                       dim3(kBlock), 0, c.st, P0->rowptr, P0->cols, P0->vals[0],
                       P0->rowblocks, M->x[1], c.sh(r), c.sh(c.t), M->dinv[0],
                       M->omega, c.sh(z), none, none, stop);
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// z (owned rows) = V-cycle(r), r ext-compact with current ghosts; two
// collectives are NOT included: the caller makes z's ghosts current.  One
// collective here: the partial coarse residuals.  gpart/rpart as vcycle().
// rc_keep != nullptr (two-launch form): the summed coarse residual C r is also
// left there (the start of the recurrences of the two-collective loop).
static int shard_vcycle(const ShardCg& c, const double* r, double* z,
                        double* gpart, double* rpart, int* nparts,
                        const double* stop, double* rc_keep = nullptr) {
  const flow_mg* M = c.G->mg;
  const flow_operator* A0 = &c.G->Ah0;
  const flow_operator* Rg = &c.G->Rg;
  const int n1 = Rg->n;
  double* const none = nullptr;
  int rc;
  if (shard_two_launch(c.G)) {
    // the rank's share of C r: its owned COLUMNS, no ghost rows involved
    if ((rc = apply(&c.G->Cg, r + (c.R->r0 - c.R->e0), c.C->buf, c.st, nullptr,
                    stop)))
      return rc;
  } else {
    // t = r - Ah r on the owned rows
    hipLaunchKernelGGL((mg_level_kernel<0, false>), dim3(A0->nblocks),
                       dim3(kBlock), 0, c.st, A0->rowptr, A0->cols, A0->vals[0],
                       A0->rowblocks, c.sh(r), c.sh(r), none, none, M->omega,
                       c.sh(c.t), none, none, stop);
    // the rank's share of the coarse residual -> buf, summed over the ranks
    if ((rc = apply(Rg, c.t + (c.R->r0 - c.R->e0), c.C->buf, c.st, nullptr, stop)))
      return rc;
  }
  if ((rc = exchange(c.C, n1))) return rc;
  if (rc_keep) {
    hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n1)), dim3(kBlock), 0, c.st, n1,
                       1.0, c.C->buf, 0.0, rc_keep);
    FLOW_CHECK_LAUNCH();
  }
  // levels >= 1: replicated
  if ((rc = vcycle(M, c.C->buf, M->x[1], c.st, nullptr, nullptr, nullptr, stop,
                   1)))
    return rc;
  return shard_up0(c, r, z, gpart, rpart, nparts, stop);
}

static size_t shard_cg_work_len(const flow_rows* R, const flow_operator* A,
                                const flow_mg_shard* G) {
  const size_t ncomp = A->kind == 4 ? 2 : 1;
  const size_t L = ncomp * (R->e1 - R->e0);
  size_t parts = G ? G->Ps0.nblocks : 0;
  if (G && G->Cg.rowptr && static_cast<size_t>(G->up_nblocks0) > parts)
    parts = G->up_nblocks0;
  return FLOW_REDUCE_WORK + (G ? 11 : 10) * L + A->nblocks + 2 + 2 * parts +
         (G && G->Cg.rowptr ? 3 * static_cast<size_t>(G->Cg.n) + 2 : 0);
}

static int shard_cg(const flow_comm* C, const flow_rows* R,
                    const flow_operator* A, const double* dinv,
                    const flow_mg_shard* G, const double* b, double* x,
                    double rtol, double atol, int maxit, int check_every,
                    int first_check, double* work, int* iters_host,
                    double* resid_host, hipStream_t st,
                    int* rejected = nullptr) {
  // rejected != nullptr: the start vector is guarded; when it is rejected,
  // *rejected = 1, x is untouched, FLOW_OK (the caller swaps in its fallback)
  if (rejected) *rejected = 0;
  ShardCg c;
  c.C = C;
  c.R = R;
  c.A = A;
  c.G = G;
  c.st = st;
  c.ncomp = A->kind == 4 ? 2 : 1;
  c.me = R->e1 - R->e0;
  c.m = R->r1 - R->r0;
  c.L = c.ncomp * c.me;
  const int L = c.L, me = c.me, n = R->n, ncomp = c.ncomp;
  c.partial = work;
  c.S = work + 3 * kRedBlocks;
  double* v = work + FLOW_REDUCE_WORK;
  c.r = v;
  c.z = c.r + L;
  c.w = c.z + L;
  c.p = c.w + L;
  c.s = c.p + L;
  c.xc = c.s + L;
  c.bc = c.xc + L;
  c.dc = c.bc + L;
  c.own = c.dc + L;
  c.t = c.own + L;                       // MG only (10 L without it)
  double* tail = c.own + L + (G ? L : 0);
  c.dpart = tail;
  c.mpart = c.dpart + A->nblocks + ((L + A->nblocks) & 1);
  const int nd = A->nblocks;
  const bool two = shard_two_launch(G);
  int nm = G ? G->Ps0.nblocks : 0;
  if (two && G->up_nblocks0 > nm) nm = G->up_nblocks0;
  // two-collective multigrid CG: the coarse images of r, s, w (replicated)
  const int n1 = two ? G->Cg.n : 0;
  double* rc_r = c.mpart + 2 * nm + (nm & 1 ? 0 : 0);
  rc_r += (reinterpret_cast<uintptr_t>(rc_r) & 15) ? 1 : 0;    // 16-byte aligned
  double* rc_s = rc_r + n1;
  double* rc_w = rc_s + n1;
  const int gl = grid_for(L);
  const int gu = grid_for(L, kBlock, kRedBlocks);
  const double rtol2 = rtol * rtol, atol2 = atol * atol;
  const double* stop = c.S + kDone;
  double* const none = nullptr;
  int rc, np = 0;

  // ext-compact copies; ownership mask
  hipLaunchKernelGGL(shard_compress_kernel, dim3(gl), dim3(kBlock), 0, st, ncomp,
                     me, R->e0, n, b, c.bc);
  hipLaunchKernelGGL(shard_compress_kernel, dim3(gl), dim3(kBlock), 0, st, ncomp,
                     me, R->e0, n, x, c.xc);
  hipLaunchKernelGGL(shard_compress_kernel, dim3(gl), dim3(kBlock), 0, st, ncomp,
                     me, R->e0, n, dinv, c.dc);
  hipLaunchKernelGGL(shard_own_kernel, dim3(gl), dim3(kBlock), 0, st, ncomp, me,
                     R->r0 - R->e0, R->r1 - R->e0, c.own);
  if ((rc = fill(kNumSlots, 0.0, c.S, st))) return rc;
  if ((rc = fill(3 * L, 0.0, c.w, st))) return rc;          // w, p, s
  // one collective per iteration: z is formed on the first ghost layer too and
  // never exchanged (rows further out stay zero)
  const bool z_local = G && shard_two_launch(G) && G->z_hi > G->z_lo;
  if (z_local && (rc = fill(L, 0.0, c.z, st))) return rc;
  FLOW_CHECK_LAUNCH();

  // |B b|^2 over the owned rows -> S[kB2] (this rank's share)
  if (G) {
    if ((rc = halo(C, R, 1, c.sh(c.bc), me, st))) return rc;
    if ((rc = shard_vcycle(c, c.bc, c.z, none, none, nullptr, nullptr)))
      return rc;
  } else {
    hipLaunchKernelGGL(vmul_kernel, dim3(gl), dim3(kBlock), 0, st, L, 1.0, c.dc,
                       c.bc, c.z);
  }
  hipLaunchKernelGGL(shard_dot2_kernel, dim3(gu), dim3(kBlock), 0, st, L, c.own,
                     c.z, c.z, c.z, c.z, c.partial, c.partial + kRedBlocks);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kBlock), 0, st, gu, 1, 0,
                     c.partial, c.S + kB2);
  FLOW_CHECK_LAUNCH();

  // r = b - A x on the owned rows, then on the ghost rows from their owners
  if ((rc = halo(C, R, ncomp, c.sh(c.xc), me, st))) return rc;
  if ((rc = apply(A, c.sh(c.xc), c.sh(c.w), st, nullptr, nullptr, me))) return rc;
  hipLaunchKernelGGL(residual_kernel, dim3(gl), dim3(kBlock), 0, st, L, c.bc, c.w,
                     static_cast<const double*>(nullptr), c.r, none);
  FLOW_CHECK_LAUNCH();
  if ((rc = halo(C, R, ncomp, c.sh(c.r), me, st))) return rc;
  // z = B r
  if (G) {
    if ((rc = shard_vcycle(c, c.r, c.z, none, none, nullptr, nullptr,
                           two ? rc_r : nullptr)))
      return rc;
    if (!z_local && (rc = halo(C, R, 1, c.sh(c.z), me, st))) return rc;
    if (two && (rc = fill(n1, 0.0, rc_s, st))) return rc;
  } else {
    hipLaunchKernelGGL(vmul_kernel, dim3(gl), dim3(kBlock), 0, st, L, 1.0, c.dc,
                       c.r, c.z);
  }
  // w = A z (owned rows, z.w partials); r.z, z.z over the owned rows
  if ((rc = apply(A, c.sh(c.z), c.sh(c.w), st, c.dpart, nullptr, me))) return rc;
  hipLaunchKernelGGL(shard_dot2_kernel, dim3(gu), dim3(kBlock), 0, st, L, c.own,
                     c.r, c.z, c.z, c.z, c.partial, c.partial + 2 * kRedBlocks);
  const int gp = 1 + grid_for(ncomp * R->nhalo > 0 ? ncomp * R->nhalo : 1,
                              kScalarBlock, 64);
  // [3 sums, |B b|^2 | (two-collective form) this rank's share of the coarse
  // image C w | halo of w]: everything that is SUMMED is a prefix, the halo
  // behind it may travel from neighbour to neighbour instead (exchange_halo)
  const int coff = 4;
  const int hoff = coff + n1;
  const int count = hoff + ncomp * R->nhalo;
  (void)count;
  // C w: the rank's owned columns
  auto coarse_image_of_w = [&](const double* flag) -> int {
    return two ? apply(&G->Cg, c.w + (R->r0 - R->e0), C->buf + coff, st, nullptr,
                       flag)
               : FLOW_OK;
  };
  if ((rc = coarse_image_of_w(nullptr))) return rc;
  hipLaunchKernelGGL(shard_finish_pack_kernel, dim3(gp), dim3(kScalarBlock), 0, st,
                     *R, ncomp, gu, nd, c.partial, c.partial + 2 * kRedBlocks,
                     c.dpart, c.S + kB2, c.sh(c.w), me, C->buf,
                     static_cast<const double*>(nullptr), hoff);
  FLOW_CHECK_LAUNCH();
  if ((rc = exchange_halo(C, R, ncomp, hoff, hoff, st))) return rc;

  const int per = R->recv_len[0] + R->recv_len[1];
  int gs = grid_for(ncomp * per > 0 ? ncomp * per : 1);
  if (two && grid_for(n1) > gs) gs = grid_for(n1);
  // alpha, beta and the verdict on the start; ghost rows of w; rc_w
  hipLaunchKernelGGL(shard_scalar_unpack_kernel, dim3(gs), dim3(kBlock), 0, st, *R,
                     ncomp, rejected ? 2 : 1, rtol2, atol2, C->buf, c.S,
                     c.sh(c.w), me, n1, coff, rc_w, hoff);
  FLOW_CHECK_LAUNCH();
  double state[kNumSlots];
  int launched = 0;
  while (true) {
    const int batch = (launched == 0 && first_check > 0) ? first_check
                                                         : check_every;
    const int todo = (maxit - launched < batch) ? maxit - launched : batch;
    for (int k = 0; k < todo; ++k) {
      const double *gpart, *rpart;
      if (G) {
        hipLaunchKernelGGL(cg_update_kernel<false>, dim3(gl), dim3(kBlock), 0, st,
                           L, c.S, c.dc, c.w, c.z, c.p, c.s, c.xc, c.r, 0,
                           c.partial, static_cast<const double*>(nullptr));
        if (two) {
          // the coarse residual by recurrence (no collective), the levels
          // >= 1 replicated, the up-sweep of level 0 on the owned rows
          hipLaunchKernelGGL(shard_rc_update_kernel, dim3(grid_for(n1)),
                             dim3(kBlock), 0, st, n1, c.S, rc_w, rc_s, rc_r);
          // Every kRcRefresh-th iteration the coarse images are recomputed
          // from the vectors they belong to, C r and C s (one more collective
          // then): carried by recurrence alone they drift away from the
          // rank-local r and s, and the preconditioner with them -- seen on a
          // 2.5 M-DoF start-up step that needs 38 iterations, where CG then
          // stagnated a factor 2.5 above its target
          if ((launched + k) % kRcRefresh == kRcRefresh - 1) {
            const int own0 = R->r0 - R->e0;
            if ((rc = apply(&G->Cg, c.r + own0, C->buf, st, nullptr, stop)))
              return rc;
            if ((rc = apply(&G->Cg, c.s + own0, C->buf + n1, st, nullptr, stop)))
              return rc;
            if ((rc = exchange(C, 2 * n1))) return rc;
            hipLaunchKernelGGL(shard_rc_refresh_kernel, dim3(grid_for(n1)),
                               dim3(kBlock), 0, st, n1, C->buf, rc_r, rc_s, stop);
          }
          if ((rc = vcycle(G->mg, rc_r, G->mg->x[1], st, nullptr, nullptr,
                           nullptr, stop, 1)))
            return rc;
          if ((rc = shard_up0(c, c.r, c.z, c.mpart, c.mpart + nm, &np, stop)))
            return rc;
        } else if ((rc = shard_vcycle(c, c.r, c.z, c.mpart, c.mpart + nm, &np,
                                      stop))) {
          return rc;
        }
        if (!z_local && (rc = halo(C, R, 1, c.sh(c.z), me, st))) return rc;
        gpart = c.mpart;
        rpart = c.mpart + nm;
      } else {
        hipLaunchKernelGGL(cg_update_kernel<true>, dim3(gu), dim3(kBlock), 0, st,
                           L, c.S, c.dc, c.w, c.z, c.p, c.s, c.xc, c.r, 1,
                           c.partial, c.own);
        np = gu;
        gpart = c.partial;
        rpart = c.partial + 2 * kRedBlocks;
      }
      if ((rc = apply(A, c.sh(c.z), c.sh(c.w), st, c.dpart, stop, me))) return rc;
      if ((rc = coarse_image_of_w(stop))) return rc;
      hipLaunchKernelGGL(shard_finish_pack_kernel, dim3(gp), dim3(kScalarBlock), 0,
                         st, *R, ncomp, np, nd, gpart, rpart, c.dpart,
                         static_cast<const double*>(nullptr), c.sh(c.w), me,
                         C->buf, stop, hoff);
      FLOW_CHECK_LAUNCH();
      if ((rc = exchange_halo(C, R, ncomp, hoff, hoff, st))) return rc;
      hipLaunchKernelGGL(shard_scalar_unpack_kernel, dim3(gs), dim3(kBlock), 0,
                         st, *R, ncomp, 0, rtol2, atol2, C->buf, c.S, c.sh(c.w),
                         me, n1, coff, rc_w, hoff);
    }
    FLOW_CHECK_LAUNCH();
    launched += todo;
    if ((rc = read_state(c.S, state, st))) return rc;
    const double res2 = state[kRes2];
    if (state[kDone] == 2.0 || !(res2 == res2)) {
      *iters_host = static_cast<int>(state[kConvIt]);
      *resid_host = res2;
      set_error("sharded CG broke down (NaN residual) at iteration %d",
                *iters_host);
      return FLOW_NOT_CONVERGED;
    }
    if (state[kDone] == 1.0) {
      *iters_host = static_cast<int>(state[kConvIt]);
      *resid_host = sqrt(res2);
      break;
    }
    if (state[kDone] == 5.0 && rejected) {
      *rejected = 1;
      *iters_host = 0;
      *resid_host = sqrt(res2);
      return FLOW_OK;
    }
    if (launched >= maxit) {
      *iters_host = launched;
      *resid_host = sqrt(res2);
      set_error("sharded CG did not converge in %d iterations: |B r| = %.3e > "
                "%.3e", launched, sqrt(res2), sqrt(state[kTarget2]));
      return FLOW_NOT_CONVERGED;
    }
  }
  // x on the owned AND ghost rows (the recurrences ran there too; z_local: on
  // the first ghost layer -- further out the search directions are zero)
  if (z_local)
    hipLaunchKernelGGL(shard_expand_kernel, dim3(grid_for(G->z_hi - G->z_lo)),
                       dim3(kBlock), 0, st, 1, G->z_hi - G->z_lo, G->z_lo, n,
                       c.xc + (G->z_lo - R->e0), x);
  else
    hipLaunchKernelGGL(shard_expand_kernel, dim3(gl), dim3(kBlock), 0, st, ncomp,
                       me, R->e0, n, c.xc, x);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}


// ---------------------------------------------------------------------------
// sharded GMRES(m): owned-compact Krylov vectors (2 * (r1 - r0) doubles), the
// operator's input staged ext-compact with its halo, block-Jacobi ILU(0)
// ---------------------------------------------------------------------------
static int shard_gmres(const flow_comm* C, const flow_rows* R,
                       const flow_operator* A, const flow_ilu* ilu,
                       const flow_pmg* pmg,
                       const double* b, double* x, double rtol, double atol,
                       int maxit, int m, int x_is_zero, int expected,
                       int verify, double* work, int* iters_host,
                       double* resid_host, hipStream_t st) {
  const int mo = R->r1 - R->r0;         // owned rows
  const int me = R->e1 - R->e0;
  const int n = R->n;
  // two components (the Newton systems: kind 3) or one (a scalar operator of
  // kind 0 on the rank's rows: the heat system)
  const int ncomp = A->kind == 0 ? 1 : 2;
  const int N = ncomp * mo;
  double* V = work + FLOW_REDUCE_WORK;
  double* Z = V + static_cast<size_t>(m + 1) * N;
  double* iwork = Z + static_cast<size_t>(m) * N;
  double* xc = iwork + N;
  double* bc = xc + N;
  double* stage = bc + N;                    // ncomp * me, ext-compact
  double* P = stage + 2 * static_cast<size_t>(me);
  double* Pww = P + kGmresMax * kRedBlocks;
  double* Pnn = Pww + kRedBlocks;
  double* G = P + FLOW_GMRES_PARTIALS;      // device state of the cycle
  double* S = work + 3 * kRedBlocks;
  const double* stop = S + kDone;
  const int gv = grid_for(N);
  const int gd = grid_for(N, kBlock, kRedBlocks);
  int rc;

  // w (owned-compact) = A v (owned-compact): stage, halo, apply on the strip
  // (the collective inside runs whatever the flag says: every rank issues the
  // same sequence)
  auto apply_owned = [&](const double* v, double* w, const double* flag) -> int {
    int r;
    if ((r = copy2d(ncomp, mo, v, mo, stage + (R->r0 - R->e0), me, st))) return r;
    if ((r = halo(C, R, ncomp, stage - R->e0, me, st))) return r;
    return apply(A, stage - R->e0, w - R->r0, st, nullptr, flag, me, mo);
  };
  // sums of nv partial lists (list k at base + k*kRedBlocks) -> all ranks'
  // total on the host
  auto sums_to_host = [&](int nparts, int nd, int extra, double* host) -> int {
    const int nv = nd + extra;
    hipLaunchKernelGGL(gmres_finish_kernel, dim3(nv), dim3(kBlock), 0, st, nparts,
                       nd, P, C->buf);
    FLOW_CHECK_LAUNCH();
    int r = exchange(C, nv);
    if (r) return r;
    return read_values(C->buf, nv, host, st);
  };

  if ((rc = copy2d(ncomp, mo, b + R->r0, n, bc, mo, st))) return rc;
  if (x_is_zero) {
    if ((rc = fill(N, 0.0, xc, st))) return rc;
  } else if ((rc = copy2d(ncomp, mo, x + R->r0, n, xc, mo, st))) {
    return rc;
  }
  if ((rc = fill(kNumSlots, 0.0, S, st))) return rc;
  // Arnoldi step j of the cycle without a read-back: the sums come out of the
  // collective summed over the ranks, the step kernel takes them from there
  // (every rank computes the same H, the same verdict)
  auto arnoldi = [&](int j, double beta, double target, bool last) -> int {
    int r;
    double* w = V + static_cast<size_t>(j + 1) * N;
    double* zj = Z + static_cast<size_t>(j) * N;
    // block Jacobi: the rank's own preconditioner on its owned rows
    if ((r = pmg ? pmg_apply(pmg, V + static_cast<size_t>(j) * N, zj, st, stop)
                 : ilu_apply(ilu, V + static_cast<size_t>(j) * N, zj, iwork, st,
                             stop)))
      return r;
    if ((r = apply_owned(zj, w, stop))) return r;
    for (int k0 = 0; k0 <= j; k0 += 8) {
      const int chunk = j + 1 - k0 < 8 ? j + 1 - k0 : 8;
#define FLOW_CALL(NV)                                                         \
  hipLaunchKernelGGL(gmres_dots_kernel<NV>, dim3(gd), dim3(kBlock), 0, st, N,  \
                     w, V + static_cast<size_t>(k0) * N,                      \
                     static_cast<size_t>(N), k0 == 0 ? 1 : 0,                 \
                     P + k0 * kRedBlocks, Pww, stop)
      FLOW_NV_SWITCH(chunk, FLOW_CALL)
#undef FLOW_CALL
    }
    const int nv = j + 2 + (j > 0 ? 1 : 0);
    hipLaunchKernelGGL(gmres_finish_kernel, dim3(nv), dim3(kBlock), 0, st, gd,
                       j + 1, P, C->buf);
    FLOW_CHECK_LAUNCH();
    if ((r = exchange(C, nv))) return r;
    hipLaunchKernelGGL(gmres_step_kernel, dim3(1), dim3(kBlock), 0, st, 0, j,
                       last ? 1 : 0, beta, target, C->buf, G, S);
    FLOW_CHECK_LAUNCH();
    if (!last &&
        (r = gmres_combine_dev(N, j + 1, G + kGCoef, G + kGCw, w, V, w, Pnn, false,
                               stop, st)))
      return r;
    return FLOW_OK;
  };

  double host[kGmresMax + 2];
  double target = 0.0, resid = 0.0;
  int it = 0;
  bool have_target = false;
  bool claimed = false;     // the last cycle stopped on the residual estimate
  while (true) {
    // r0 = b - A x -> V_0
    if (x_is_zero && it == 0) {
      hipLaunchKernelGGL(axpby_kernel, dim3(gv), dim3(kBlock), 0, st, N, 1.0, bc,
                         0.0, V);
    } else {
      if ((rc = apply_owned(xc, iwork, nullptr))) return rc;
      hipLaunchKernelGGL(residual_kernel, dim3(gv), dim3(kBlock), 0, st, N, bc,
                         iwork, static_cast<const double*>(nullptr), V,
                         static_cast<double*>(nullptr));
    }
    // |b|^2 and |r0|^2 in one collective (lists 0 and 1 of P)
    hipLaunchKernelGGL(gmres_dots_kernel<1>, dim3(gd), dim3(kBlock), 0, st, N, bc,
                       bc, static_cast<size_t>(N), 0, P, Pww,
                       static_cast<const double*>(nullptr));
    hipLaunchKernelGGL(gmres_dots_kernel<1>, dim3(gd), dim3(kBlock), 0, st, N, V,
                       V, static_cast<size_t>(N), 0, P + kRedBlocks, Pww,
                       static_cast<const double*>(nullptr));
    FLOW_CHECK_LAUNCH();
    if ((rc = sums_to_host(gd, 2, 0, host))) return rc;
    if (!have_target) {
      target = fmax(rtol * sqrt(host[0]), atol);
      have_target = true;
      // a start vector that leaves a larger residual than zero would is
      // dropped (every rank sees the same sums): V_0 = b, x = 0
      if (!x_is_zero && host[1] > host[0]) {
        hipLaunchKernelGGL(axpby_kernel, dim3(gv), dim3(kBlock), 0, st, N, 1.0, bc,
                           0.0, V);
        if ((rc = fill(N, 0.0, xc, st))) return rc;
        host[1] = host[0];
      }
    }
    const double res2 = host[1];
    const double beta = sqrt(res2);
    resid = beta;
    if (!(res2 == res2)) {
      *iters_host = it;
      *resid_host = res2;
      set_error("sharded GMRES broke down (NaN residual) at iteration %d", it);
      return FLOW_NOT_CONVERGED;
    }
    // (behind a cycle that stopped on the estimate: the verification with the
    // true residual, as gmres() -- every rank sees the same sums)
    if (beta <= target || (claimed && beta <= 10.0 * target)) break;
    claimed = false;
    if (it >= maxit) {
      *iters_host = it;
      *resid_host = beta;
      set_error("sharded GMRES did not converge in %d iterations: |r| = %.3e > "
                "%.3e", it, beta, target);
      return FLOW_NOT_CONVERGED;
    }

    // one cycle (as gmres(): the plan only depends on numbers every rank has)
    const int it0 = it;
    int enq = 0, cols = 0;
    bool converged = false;
    double state[kNumSlots];
    while (true) {
      const int room = (m < maxit - it0 ? m : maxit - it0) - enq;
      if (room <= 0) break;
      int plan = expected - (it0 + enq);
      if (plan < 1) plan = 1;
      if (plan > room) plan = room;
      for (int k = 0; k < plan; ++k, ++enq) {
        const bool last = enq + 1 >= m || it0 + enq + 1 >= maxit;
        if ((rc = arnoldi(enq, beta, target, last))) return rc;
      }
      if ((rc = read_state(S, state, st))) return rc;
      cols = static_cast<int>(state[kConvIt]);
      if (state[kDone] == 2.0) {
        *iters_host = it0 + cols;
        *resid_host = resid;
        set_error("sharded GMRES broke down (NaN) at iteration %d", it0 + cols);
        return FLOW_NOT_CONVERGED;
      }
      resid = state[kRes2];
      if (state[kDone] != 0.0) {
        converged = state[kDone] == 1.0;   // 3: verify with the true residual
        break;
      }
    }
    it = it0 + cols;
    if ((rc = fill(1, 0.0, S + kDone, st))) return rc;
    if (cols > 0 &&
        (rc = gmres_combine_dev(N, cols, G + kGYc, nullptr, nullptr, Z, xc,
                                nullptr, true, nullptr, st)))
      return rc;
    x_is_zero = 0;
    if (converged && !verify) break;
    claimed = converged;
  }
  // the owned rows of x
  if ((rc = copy2d(ncomp, mo, xc, mo, x + R->r0, n, st))) return rc;
  *iters_host = it;
  *resid_host = resid;
  return FLOW_OK;
}

}  // namespace flow

extern "C" int flow_shard_halo(const flow_comm* comm, const flow_rows* rows,
                               int ncomp, double* x, int stride, void* stream) {
  int rc = check_rows(rows);
  if (rc) return rc;
  FLOW_REQUIRE(ncomp == 1 || ncomp == 2, "components");
  if ((rc = check_comm(comm, static_cast<long long>(ncomp) * rows->nhalo)))
    return rc;
  FLOW_REQUIRE(x != nullptr && stride >= rows->e1 - rows->e0, "halo vector");
  return halo(comm, rows, ncomp, x, stride, as_stream(stream));
}

extern "C" int flow_shard_reduce_host(const flow_comm* comm,
                                      const flow_rows* rows, int ncomp,
                                      const double* x, const double* y,
                                      int stride, int kind, double* work,
                                      double* result_host, void* stream) {
  int rc = check_rows(rows);
  if (rc) return rc;
  if ((rc = check_comm(comm, kNumSlots))) return rc;
  FLOW_REQUIRE(ncomp == 1 || ncomp == 2, "components");
  FLOW_REQUIRE(x && work && result_host && (kind == 1 || y), "reduce arguments");
  FLOW_REQUIRE(kind == 0 || kind == 1, "reduce kind");
  hipStream_t st = as_stream(stream);
  const int m = rows->r1 - rows->r0;
  const double* x0 = x + rows->r0;
  const double* x1 = x0 + (ncomp == 2 ? stride : 0);
  double host[kNumSlots];
  if (kind == 0) {
    const double* y0 = y + rows->r0;
    const double* y1 = y0 + (ncomp == 2 ? stride : 0);
    int np = 0;
    if ((rc = dots(m, ncomp, x0, y0, x1, y1, x0, y0, work, &np, st))) return rc;
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kBlock), 0, st, np, ncomp, 0,
                       work, comm->buf);
    FLOW_CHECK_LAUNCH();
    if ((rc = exchange(comm, ncomp))) return rc;
    if ((rc = read_values(comm->buf, ncomp, host, st))) return rc;
    *result_host = host[0] + (ncomp == 2 ? host[1] : 0.0);
    return FLOW_OK;
  }
  double* S = work + 3 * kRedBlocks;
  const int g = grid_for(m, kBlock * 4, kRedBlocks);
  for (int a = 0; a < ncomp; ++a) {
    hipLaunchKernelGGL(absmax_kernel, dim3(g), dim3(kBlock), 0, st, m,
                       a == 0 ? x0 : x1, work);
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kBlock), 0, st, g, 1, 1, work,
                       S + a);
  }
  hipLaunchKernelGGL(shard_rank_slot_kernel, dim3(1), dim3(64), 0, st, comm->world,
                     comm->rank, ncomp, S, comm->buf);
  FLOW_CHECK_LAUNCH();
  if ((rc = exchange(comm, comm->world))) return rc;
  if ((rc = read_values(comm->buf, comm->world, host, st))) return rc;
  double mx = 0.0;
  for (int k = 0; k < comm->world; ++k) mx = fmax(mx, host[k]);
  *result_host = mx;
  return FLOW_OK;
}

static int check_shard_solver(const flow_comm* comm, const flow_rows* rows,
                              const flow_operator* A, const double* b,
                              const double* x, double rtol, double atol,
                              int maxit, const double* work,
                              const int* iters_host, const double* resid_host) {
  int rc = check_rows(rows);
  if (rc) return rc;
  if ((rc = check_operator(A))) return rc;
  FLOW_REQUIRE(A->n == rows->n, "operator / row ranges");
  FLOW_REQUIRE(b && x && work && iters_host && resid_host, "solver pointers");
  FLOW_REQUIRE(rtol >= 0.0 && atol >= 0.0 && maxit >= 0, "solver tolerances");
  FLOW_REQUIRE(reinterpret_cast<uintptr_t>(work) % 16 == 0,
               "solver workspace must be 16-byte aligned");
  (void)comm;
  return FLOW_OK;
}

extern "C" int flow_shard_cg_solve(const flow_comm* comm, const flow_rows* rows,
                                   const flow_operator* A, const double* dinv,
                                   const double* b, double* x, double rtol,
                                   double atol, int maxit, int check_every,
                                   int first_check, double* work,
                                   size_t work_len, int* iters_host,
                                   double* resid_host,
                                   int* start_rejected_host, void* stream) {
  int rc = check_shard_solver(comm, rows, A, b, x, rtol, atol, maxit, work,
                              iters_host, resid_host);
  if (rc) return rc;
  FLOW_REQUIRE(A->kind == 0 || A->kind == 4, "sharded CG: operator kind 0 or 4");
  FLOW_REQUIRE(dinv != nullptr && check_every > 0 && first_check >= 0,
               "sharded CG arguments");
  const int ncomp = A->kind == 4 ? 2 : 1;
  if ((rc = check_comm(comm, 4 + static_cast<long long>(ncomp) * rows->nhalo)))
    return rc;
  FLOW_REQUIRE(work_len >= shard_cg_work_len(rows, A, nullptr),
               "sharded CG workspace too small");
  return shard_cg(comm, rows, A, dinv, nullptr, b, x, rtol, atol, maxit,
                  check_every, first_check, work, iters_host, resid_host,
                  as_stream(stream), start_rejected_host);
}

extern "C" int flow_shard_mgcg_solve(
    const flow_comm* comm, const flow_rows* rows, const flow_operator* A,
    const double* dinv, const flow_mg_shard* mgs, const double* b, double* x,
    double rtol, double atol, int maxit, int check_every, int first_check,
    double* work, size_t work_len, int* iters_host, double* resid_host,
    int* start_rejected_host, void* stream) {
  int rc = check_shard_solver(comm, rows, A, b, x, rtol, atol, maxit, work,
                              iters_host, resid_host);
  if (rc) return rc;
  FLOW_REQUIRE(A->kind == 0 && dinv != nullptr && check_every > 0 &&
                   first_check >= 0,
               "sharded multigrid CG arguments");
  FLOW_REQUIRE(mgs && mgs->mg, "sharded hierarchy");
  if ((rc = check_mg(mgs->mg, A->n))) return rc;
  FLOW_REQUIRE(mgs->mg->nlevels >= 2, "multigrid: at least two levels");
  if ((rc = check_operator(&mgs->Ah0))) return rc;
  if ((rc = check_operator(&mgs->Ps0))) return rc;
  if ((rc = check_operator(&mgs->Rg))) return rc;
  FLOW_REQUIRE(mgs->Ah0.kind == 0 && mgs->Ps0.kind == 0 && mgs->Rg.kind == 0 &&
                   mgs->Ah0.n == A->n && mgs->Ps0.n == A->n &&
                   mgs->Rg.n == mgs->mg->R[0].n,
               "sharded hierarchy operators");
  long long need = 4 + rows->nhalo;
  if (mgs->Cg.rowptr) {
    if ((rc = check_operator(&mgs->Cg))) return rc;
    FLOW_REQUIRE(mgs->mg->C[0].rowptr && mgs->Cg.kind == 0 &&
                     mgs->Cg.n == mgs->Rg.n && mgs->up_rowblocks0 &&
                     mgs->up_nblocks0 > 0,
                 "sharded hierarchy: two-launch form");
    need += mgs->Cg.n;
    if (2LL * mgs->Cg.n > need) need = 2LL * mgs->Cg.n;
    FLOW_REQUIRE(mgs->z_hi <= mgs->z_lo ||
                     (mgs->z_lo >= rows->e0 && mgs->z_lo <= rows->r0 &&
                      mgs->z_hi >= rows->r1 && mgs->z_hi <= rows->e1),
                 "sharded hierarchy: [z_lo, z_hi) must hold the owned rows and "
                 "lie inside the rows' window");
  }
  if (mgs->Rg.n > need) need = mgs->Rg.n;
  if ((rc = check_comm(comm, need))) return rc;
  FLOW_REQUIRE(work_len >= shard_cg_work_len(rows, A, mgs),
               "sharded multigrid CG workspace too small");
  return shard_cg(comm, rows, A, dinv, mgs, b, x, rtol, atol, maxit, check_every,
                  first_check, work, iters_host, resid_host, as_stream(stream),
                  start_rejected_host);
}

extern "C" int flow_shard_gmres_solve(
    const flow_comm* comm, const flow_rows* rows, const flow_operator* A,
    const flow_ilu* ilu, const flow_pmg* pmg, const double* b, double* x,
    double rtol, double atol, int maxit, int restart, int x_is_zero,
    int expected_its, int verify, double* work, size_t work_len,
    int* iters_host, double* resid_host, void* stream) {
  int rc = check_shard_solver(comm, rows, A, b, x, rtol, atol, maxit, work,
                              iters_host, resid_host);
  if (rc) return rc;
  FLOW_REQUIRE(A->kind == 3 || A->kind == 0,
               "sharded GMRES: the matrix-free Jacobian action (kind 3) or a "
               "scalar operator on the rank's rows (kind 0)");
  if ((rc = check_gmres_args(restart, expected_its))) return rc;
  const int ncomp = A->kind == 0 ? 1 : 2;
  if (A->kind == 3) {
    const flow_momentum_jvp* J =
        static_cast<const flow_momentum_jvp*>(A->matfree);
    FLOW_REQUIRE(J->W->r0 == rows->r0 && J->W->r1 == rows->r1,
                 "the operator's row range must be the rank's owned rows");
  }
  const int mo = rows->r1 - rows->r0, me = rows->e1 - rows->e0;
  FLOW_REQUIRE((ilu != nullptr) != (pmg != nullptr),
               "sharded GMRES needs ONE block-Jacobi preconditioner: ilu or pmg");
  FLOW_REQUIRE(pmg == nullptr || ncomp == 2,
               "the p-multigrid cycle is a two-component preconditioner");
  if (ilu && (rc = ilu_check(ilu, ncomp * mo))) return rc;
  if (pmg && (rc = pmg_check(pmg, 2 * mo))) return rc;
  long long need = static_cast<long long>(ncomp) * rows->nhalo;
  if (need < FLOW_GMRES_MAX_RESTART + 2) need = FLOW_GMRES_MAX_RESTART + 2;
  if ((rc = check_comm(comm, need))) return rc;
  FLOW_REQUIRE(work_len >= FLOW_REDUCE_WORK +
                               (2 * static_cast<size_t>(restart) + 4) * ncomp * mo +
                               2 * static_cast<size_t>(me) + FLOW_GMRES_PARTIALS +
                               FLOW_GMRES_STATE,
               "sharded GMRES workspace too small");
  return shard_gmres(comm, rows, A, ilu, pmg, b, x, rtol, atol, maxit, restart,
                     x_is_zero, expected_its, verify, work, iters_host,
                     resid_host, as_stream(stream));
}
