// lmpc_pbt.h -- launch arguments of the exploit/explore step of population-based training (lmpc_pbt.hip,
// dart_lmpc_pbt_step_dev): the P learners of dart_lmpc_train_pop are ranked by a figure of merit that lies on the
// device, the k worst restart from the nets, the optimizer state and the hyper-parameters of one of the k best, and
// their hyper-parameters are perturbed.  Two plain launches in stream order: the rank kernel (one wave) writes the
// ranks, the parents and the children's rows of the hyper-parameter table; the copy kernel streams the parents' rows
// into the children's.  The parent table travels between them in parent_out.  No atomics, no cooperative launch, no
// loop that waits on memory; no donor is a child (2 k <= P), so no row is read and written in one launch.
//
// The rule, exact (dart_mpc/ppo.py pbt_plan states it in numpy, bit for bit):
//   ranking  a is better than b if its fitness is strictly better in the configured direction, or the two compare
//            equal and a < b; a NaN is worse than every non-NaN, NaNs are ordered among themselves by index, +-inf
//            are ordinary values.  rank[l] = the number of learners better than l.
//   exploit  children: rank >= P - k; donors: ranks 0 .. k - 1.  Child l takes the Philox4x32-10 block at counter
//            (l, generation, kStreamPbt, 0), key (seed & 0xffffffff, seed >> 32); its parent is the learner of rank
//            word0 % k.  parent[l] = l for everyone else.
//   explore  children only, column c: v = hyper[parent][c]; with bit c of explore_mask, v = v * (w >> 31 ? factor_up
//            : factor_down), w = word c % 4 of the block at counter (l, generation, kStreamPbt, 1 + c / 4), one fp64
//            product; then v < lo[c] ? lo[c] : (v > hi[c] ? hi[c] : v), so a NaN passes through; hyper[l][c] = v.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmpc_ppo.h"
#include "lmpc_train.h"

namespace dartmpc {

struct PbtRankArgs {            // one wave64, learner l on lane l
    int P, k;                   // 1 <= P <= kPopMax, 0 <= 2 k <= P (k = 0: ranks and parent = self alone)
    int higher_is_better;
    long long fitness_stride;   // >= 1, in doubles
    uint32_t key0, key1, generation, explore_mask;
    double factor_down, factor_up;
    double lo[kHyperCols], hi[kHyperCols];
    const double* fitness;      // learner l's at fitness[l * fitness_stride]
    double* hyper;              // [P][kHyperCols] in/out: the children's rows are written
    int32_t* rank_out;          // [P]
    int32_t* parent_out;        // [P]
};

// grid (chunks, P): the blocks of learner y return at once when parent[y] is y (or no learner); the others copy the
// parent's actor row, its 37569 critic weights (the pad floats of a row are neither read nor written), both Adam
// moments and its step count into learner y's, bit for bit, in 16-byte moves where both rows are 16-byte aligned
// (actor and critic rows are when their bases are; a learner's adam row [2][77317] is not for odd l) and in 8- or
// 4-byte moves elsewhere
struct PbtCopyArgs {
    int P;
    const int32_t* parent;      // [P], the rank kernel's
    float* weights;             // [P][39748]
    float* critic;              // [P][kPopCriticStride]
    float* adam;                // [P][2][77317]
    int32_t* adam_step;         // [P]
};

constexpr int kPbtCopyThreads = 256, kPbtCopyChunks = 32;

}  // namespace dartmpc

extern "C" hipError_t dartmpc_launch_lmpc_pbt_rank(const dartmpc::PbtRankArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_pbt_copy(const dartmpc::PbtCopyArgs* args, hipStream_t stream);
