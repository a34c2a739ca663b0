// pairs_bin_index.h -- the counting sort of a (pair, level)'s points into square bins, ONCE for the kernels that build such an
// index (pairs_smooth.hip: k_pairs_smooth_index over the level's keypoints; pairs_carry.hip: k_pairs_carry_index over the carried
// points of the level).  One workgroup of 256 lanes per (pair, level).  A kernel is bin_index(members, K, ...) with `members` its
// policy, as the keypoint kernels take their camera:
//
//   members.at(i, x, y)     candidate i < K: false if it is no member of the index, else true and its whole pixel in (x, y)
//   Members::kEvery         true: every candidate is a member (at never returns false), and the members' total is K
//
// Each of the four waves owns a contiguous range of candidate indices and a histogram of its own in LDS: counts by integer LDS
// atomics, one exclusive scan over (bin, wave) -- which turns histogram [w][c] into the first place of wave w's members of bin c --
// then the scatter, a wave walking its range in ascending steps of 64 and ranking the lanes of a step that share a bin by a ballot.
// Nothing decides a place but the candidate's index: within a bin the members are ascending.  Count and scatter ask the policy the
// same question of the same stored value, so a place is below the total the counts gave.
#ifndef MBAVO_PAIRS_BIN_INDEX_H
#define MBAVO_PAIRS_BIN_INDEX_H

#include "pairs_prep.h"
#include "pairs_desc.h"
#include <hip/hip_runtime.h>

namespace mbavo
{
    namespace pairs
    {
        constexpr int kIndexWaves = 4;

        __device__ __forceinline__ int smooth_bin(int x, int y, int s, int nbx, int nby)
        { // (a keypoint lies inside its level's image; the clamps keep a foreign coordinate inside the tables all the same)
            int bx = x / s, by = y / s;
            bx = bx < 0 ? 0 : (bx >= nbx ? nbx - 1 : bx);
            by = by < 0 ? 0 : (by >= nby ? nby - 1 : by);
            return by * nbx + bx;
        }

        // the bin edge of a level of W x H pixels: the smallest s >= radius with at most kSmoothBins bins
        __host__ __device__ inline int bin_edge(int radius, int W, int H)
        {
            int s = radius;
            while ((long long)((W + s - 1) / s) * ((H + s - 1) / s) > kSmoothBins) ++s;
            return s;
        }

        // Where an index over all (pair, level)s lies in its owner's allocation: [bin starts B x L x kSmoothStarts ints | perm |
        // pxy | the owner's own arrays from o_tail on], perm and pxy one entry per slot (pairs_prep.h: DepthSlots), every array
        // 256-byte aligned
        struct IndexLayout
        {
            long long o_perm, o_pxy, o_tail;
            int *starts(char *b) const { return (int *)b; }
            int *perm(char *b) const { return (int *)(b + o_perm); }
            SmoothXY *pxy(char *b) const { return (SmoothXY *)(b + o_pxy); }
        };
        inline IndexLayout index_layout(const PairsPlan &p, size_t n_slots)
        {
            IndexLayout ix;
            ix.o_perm = align_up((long long)sizeof(int) * kSmoothStarts * p.B * p.L, kAlign);
            ix.o_pxy = ix.o_perm + align_up((long long)sizeof(int) * (long long)n_slots, kAlign);
            ix.o_tail = ix.o_pxy + align_up((long long)sizeof(SmoothXY) * (long long)n_slots, kAlign);
            return ix;
        }
        // the dynamic LDS of an index kernel at `radius`: kIndexWaves histograms over the most bins of a reported level (-1: any)
        inline size_t index_lds(const PairsPlan &p, int radius, int level)
        {
            int bins_max = 1;
            for (int l = 0; l < p.L; ++l)
                if (level < 0 || level == l)
                {
                    const int s = bin_edge(radius, p.W[l], p.H[l]), nb = ((p.W[l] + s - 1) / s) * ((p.H[l] + s - 1) / s);
                    bins_max = nb > bins_max ? nb : bins_max;
                }
            return sizeof(int) * (size_t)kIndexWaves * bins_max;
        }

        // s_hist: kIndexWaves x nb ints of LDS; s_wave: 4 ints of LDS; starts: nb + 1 ints; perm, pxy: one entry per member
        template <class Members>
        __device__ __forceinline__ void bin_index(const Members m, int K, int s, int nbx, int nby, int *__restrict__ starts, int *__restrict__ perm,
                                                  SmoothXY *__restrict__ pxy, int *s_hist, int *s_wave)
        {
            const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int nb = nbx * nby; // <= kSmoothBins (the host chose s so)
            int *hist = s_hist + wave * nb;

            for (int c = tid; c < kIndexWaves * nb; c += 256) s_hist[c] = 0;
            __syncthreads();
            // ---- counts: wave w owns the steps [w per_wave, (w + 1) per_wave) of 64 candidates
            const int steps = (K + 63) / 64, per_wave = (steps + kIndexWaves - 1) / kIndexWaves;
            const int step0 = wave * per_wave, step1 = step0 + per_wave < steps ? step0 + per_wave : steps;
            for (int st = step0; st < step1; ++st)
            {
                const int i = st * 64 + lane;
                if (i < K)
                {
                    int x, y;
                    if (m.at(i, x, y)) atomicAdd(&hist[smooth_bin(x, y, s, nbx, nby)], 1);
                }
            }
            __syncthreads();
            // ---- the exclusive scan over (bin, wave): a thread takes `per` consecutive bins
            const int per = (nb + 255) / 256, c0 = tid * per, c1 = c0 + per < nb ? c0 + per : nb;
            int mine = 0;
            for (int c = c0; c < c1; ++c)
                for (int w = 0; w < kIndexWaves; ++w) mine += s_hist[w * nb + c];
            int incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1)
            {
                const int v = __shfl_up(incl, off);
                if (lane >= off) incl += v;
            }
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            int run = incl - mine;
            for (int w = 0; w < wave; ++w) run += s_wave[w];
            for (int c = c0; c < c1; ++c)
            {
                starts[c] = run;
                for (int w = 0; w < kIndexWaves; ++w)
                {
                    const int n = s_hist[w * nb + c];
                    s_hist[w * nb + c] = run;
                    run += n;
                }
            }
            if constexpr (Members::kEvery)
            {
                if (tid == 0) starts[nb] = K;
            }
            else
            {
                if (tid == 255) starts[nb] = run; // (the last thread's running place behind its bins: the members' total)
            }
            __syncthreads();
            // ---- the scatter, stable by construction
            for (int st = step0; st < step1; ++st)
            {
                const int i = st * 64 + lane;
                int x = 0, y = 0, bin = -1;
                const bool active = i < K && m.at(i, x, y);
                if (active) bin = smooth_bin(x, y, s, nbx, nby);
                unsigned long long todo = __ballot(active);
                while (todo != 0)
                {
                    const int leader = __ffsll((long long)todo) - 1;
                    const int c = __shfl(bin, leader);
                    const unsigned long long same = __ballot(active && bin == c);
                    const int base = hist[c]; // (every lane reads it before the leader moves it on)
                    if (active && bin == c)
                    {
                        const int pos = base + __popcll(same & ((1ull << lane) - 1ull)); // < the total: the counts of the first pass
                        perm[pos] = i;
                        pxy[pos] = SmoothXY{x, y};
                    }
                    if (lane == leader) hist[c] = base + __popcll(same);
                    todo &= ~same;
                }
            }
        }
    } // namespace pairs
} // namespace mbavo

#endif
