// lmpc_pbt.hip -- the exploit/explore step of population-based training on the device (lmpc_pbt.h states the
// rule): lmpc_pbt_rank_kernel ranks the learners by wave-wide comparison, draws the children's parents and writes
// their rows of the hyper-parameter table; lmpc_pbt_copy_kernel streams the parents' nets and optimizer state into
// the children's.  Plain launches in stream order.
#include "lmpc_pbt.h"

namespace dartmpc {

// true when learner j (fitness fj) is better than learner l (fitness fl)
__device__ __forceinline__ bool pbt_better(double fj, int j, double fl, int l, bool higher) {
    const bool nj = fj != fj, nl = fl != fl;
    if (nj || nl) return nj ? (nl && j < l) : true;
    const bool strict = higher ? fj > fl : fj < fl;
    return strict || (fj == fl && j < l);
}

__global__ __launch_bounds__(64) void lmpc_pbt_rank_kernel(PbtRankArgs a) {
    const int l = threadIdx.x;
    const bool live = l < a.P;
    const double f = live ? a.fitness[(long long)l * a.fitness_stride] : 0.0;
    const bool higher = a.higher_is_better != 0;
    // every lane walks the P learners (the trip count is the launch's, never the table's)
    int rank = 0;
    for (int j = 0; j < a.P; ++j) {
        const double fj = __shfl(f, j);
        if (pbt_better(fj, j, f, l, higher)) ++rank;
    }
    const bool child = live && a.k > 0 && rank >= a.P - a.k;
    int want = -1;
    if (child) want = (int)(philox4x32_10((uint32_t)l, a.generation, kStreamPbt, 0u, a.key0, a.key1).w[0] % (uint32_t)a.k);
    int parent = l;
    for (int j = 0; j < a.P; ++j) {
        const int rj = __shfl(rank, j);
        if (child && rj == want) parent = j;
    }
    if (live) {
        a.rank_out[l] = rank;
        a.parent_out[l] = parent;
    }
    if (!child) return;
    // (a parent's rank is below k <= P - k: no parent is a child, so no row read here is written here)
    const double* src = a.hyper + (size_t)parent * kHyperCols;
    double* dst = a.hyper + (size_t)l * kHyperCols;
    Philox4 blk[(kHyperCols + 3) / 4];
#pragma unroll
    for (int q = 0; q < (kHyperCols + 3) / 4; ++q)
        blk[q] = philox4x32_10((uint32_t)l, a.generation, kStreamPbt, 1u + q, a.key0, a.key1);
#pragma unroll
    for (int c = 0; c < kHyperCols; ++c) {
        double v = src[c];
        if ((a.explore_mask >> c) & 1u) v = v * ((blk[c / 4].w[c % 4] >> 31) ? a.factor_up : a.factor_down);
        v = v < a.lo[c] ? a.lo[c] : (v > a.hi[c] ? a.hi[c] : v);
        dst[c] = v;
    }
}

// n 32-bit words from src to dst in moves of V, the tail in single words; thread `first` of `stride`
template <class V>
__device__ __forceinline__ void pbt_copy_as(uint32_t* dst, const uint32_t* src, int n, int first, int stride) {
    constexpr int W = sizeof(V) / sizeof(uint32_t);
    const int nv = n / W;
    V* d = reinterpret_cast<V*>(dst);
    const V* s = reinterpret_cast<const V*>(src);
    for (int i = first; i < nv; i += stride) d[i] = s[i];
    for (int i = nv * W + first; i < n; i += stride) dst[i] = src[i];
}

__device__ __forceinline__ void pbt_copy_row(float* dst, const float* src, int n, int first, int stride) {
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    const uintptr_t both = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src);    // block-uniform
    if ((both & 15) == 0) pbt_copy_as<uint4>(d, s, n, first, stride);
    else if ((both & 7) == 0) pbt_copy_as<uint2>(d, s, n, first, stride);
    else pbt_copy_as<uint32_t>(d, s, n, first, stride);
}

__global__ __launch_bounds__(kPbtCopyThreads) void lmpc_pbt_copy_kernel(PbtCopyArgs a) {
    const int l = blockIdx.y;
    if (l >= a.P) return;
    const int par = a.parent[l];
    if (par == l || par < 0 || par >= a.P) return;          // a survivor (or no learner): block-uniform
    const int first = blockIdx.x * kPbtCopyThreads + threadIdx.x, stride = gridDim.x * kPbtCopyThreads;
    const size_t c = (size_t)l, p = (size_t)par;
    pbt_copy_row(a.weights + c * kPpoActorN, a.weights + p * kPpoActorN, kPpoActorN, first, stride);
    pbt_copy_row(a.critic + c * kPopCriticStride, a.critic + p * kPopCriticStride, kPpoCriticN, first, stride);
    pbt_copy_row(a.adam + c * 2 * (size_t)kPpoParams, a.adam + p * 2 * (size_t)kPpoParams, 2 * kPpoParams, first, stride);
    if (first == 0) a.adam_step[l] = a.adam_step[par];
}

}  // namespace dartmpc

extern "C" hipError_t dartmpc_launch_lmpc_pbt_rank(const dartmpc::PbtRankArgs* args, hipStream_t stream) {
    if (args->P <= 0) return hipSuccess;
    hipLaunchKernelGGL(dartmpc::lmpc_pbt_rank_kernel, dim3(1), dim3(64), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_pbt_copy(const dartmpc::PbtCopyArgs* args, hipStream_t stream) {
    if (args->P <= 0) return hipSuccess;
    hipLaunchKernelGGL(dartmpc::lmpc_pbt_copy_kernel, dim3(dartmpc::kPbtCopyChunks, args->P),
                       dim3(dartmpc::kPbtCopyThreads), 0, stream, *args);
    return hipGetLastError();
}
