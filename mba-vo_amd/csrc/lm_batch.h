// lm_batch.h -- the batched Levenberg-Marquardt loop (lm_batch.hip): the LM loop of tracker.cpp for B pairs of L pyramid levels
// each (probs: B x L, pair-major; L = 1: one-level problems), coarse to fine, with all control state on the device.
#ifndef MBAVO_LM_BATCH_H
#define MBAVO_LM_BATCH_H

#include "engine.h"

namespace mbavo
{
    // What a GROUP of a bigger batch takes from the whole batch (c_api.cpp: mbavo_lm_batch) so that every group runs the same
    // kernel form with the same strides: the largest knot count and the largest sample count of a list.
    struct LmBatchShared
    {
        int max_N = 0, max_S = 1;
        static LmBatchShared of(const mbavo_problem *probs, int count)
        {
            LmBatchShared s;
            for (int b = 0; b < count; ++b)
            {
                s.max_N = probs[b].N > s.max_N ? probs[b].N : s.max_N;
                s.max_S = probs[b].S > s.max_S ? probs[b].S : s.max_S;
            }
            return s;
        }
    };
    int lm_batch(Engine &eng, int B, int L, const mbavo_problem *probs, const mbavo_lm_batch_opts &opt, mbavo_lm_batch_result *results,
                 mbavo_trace_rec *trace, int trace_cap, const LmBatchShared *shared = nullptr);
    // the argument rules of lm_batch for the whole batch (0 or MBAVO_E_ARG), checked before any group of it is started
    int lm_batch_check(int B, int L, const mbavo_problem *probs, const mbavo_lm_batch_opts &opt);
}

#endif
