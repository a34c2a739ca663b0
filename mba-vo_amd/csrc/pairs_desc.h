// pairs_desc.h -- what the parts of a batch of keyframe pairs share on the device (pairs_prep.hip: the images and keypoints;
// pairs_track.hip: the tracker; pairs_report.hip: the report; pairs_hyp.hip: the motion hypotheses; pairs_refine.hip, pairs_filter.hip,
// pairs_search.hip, pairs_smooth.hip, pairs_carry.hip, pairs_prune.hip: the depth refinement, filter, search, smoothing, hand-over and pruning): one (pair, level) of the device-resident table, the alignment of the arena's arrays, the tracker state's layout,
// the report, hypothesis, refinement and filter kernels' arguments and the spline sample that tracker and report both take at the capture
// time.
#ifndef MBAVO_PAIRS_DESC_H
#define MBAVO_PAIRS_DESC_H

#include "../../include/mbavo.h"
#include "se3_math.h"

namespace mbavo
{
    struct CellPick; // vo_frontend.h

    struct PairLevelDesc
    {
        unsigned char *ref, *cur; // this level of the keyframe / the current frame
        void *grad;               // float2 / __half2 / packed word per pixel
        double *kp_xy, *kp_z;
        union
        {
            CellPick *picks;      // grid selection: `cells` of them
            int *seg;             // every candidate: one int per 256 pixels (candidate count, then its exclusive scan)
        };
        int H, W, ch, cw, cells_w, cells, border;
        int clear0;               // mbavo_pairs_opts.valid_radius > 0: first byte of this level within a camera's clearance pyramid
        double scale;             // 2^level
    };

    // where the levels start in the grids that run over all levels of a pair (by value: L <= 8)
    struct PairsGrid
    {
        int L, B;
        int blk0[9];  // gradients, corner scores: first workgroup of every level
        int cell0[9]; // grid selection: first cell of every level; every candidate: first workgroup (1024 pixels) of every level
    };

    namespace pairs
    {
        // the corner scores of an object (mbavo_pairs_set_detector; pairs_score.hip): one float per pixel, laid out as the gradient
        // slices are -- the slice of a (pair, level) starts as many pixels behind `base` as its gradient slice starts behind the
        // first one, so the table names it without a word of its own
        struct ScoreSlices
        {
            float *base;
            const char *grad0; // the gradients of pair 0, level 0
            int shift;         // log2 of the gradient bytes per pixel
#if defined(__HIPCC__)
            __device__ __forceinline__ float *of(const PairLevelDesc &d) const { return base + (((const char *)d.grad - grad0) >> shift); }
#endif
        };

        constexpr long long kAlign = 256;
        inline long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

        // the pair of a grid row: the row itself in a prepare (no list), the row's entry of the key list in an update.  Uniform
        // over the grid, decided by a kernel argument.
        __device__ __forceinline__ int pair_of_row(const int *key_pairs, int row) { return key_pairs ? key_pairs[row] : row; }

        // what k_pairs_report reads and writes (pairs_report.hip): the level-0 evaluation of all pairs in the object's report
        // scratch, the motion as the LM left it, the caller's optional arrays
        struct ReportArgs
        {
            const int *counts;            // B x L: level 0 of pair b at b * L
            const double *cap, *t0;       // B each
            const double *kt, *kR;        // B x 3N, B x 4N
            const double *blocks;         // B packed frame blocks [cost | g_local | upper(H_local)]
            const double *patch_cost;     // the evaluation's patch costs, pair after pair without gaps: pair b's K start at sum of the K before it
            const double *valid;          // B in-bounds pixel counts
            double dt, chi;
            int L, N, P, cap0;            // P: level 0's patch size; cap0: level 0's keypoint capacity
            struct mbavo_pairs_report *out; // B
            double *patch_cost_out;       // B x cap0, or null
            unsigned char *flags_out;     // B x cap0, or null
        };

        // the tracker state of a pair on the device (pairs_track.hip writes it; pairs_hyp.hip reads velocity and prev_timestamp
        // and leaves dt_frame as the predict does): kStateLen doubles
        constexpr int kStateKeyframe = 0, kStatePrev = 7, kStateVelocity = 14, kStatePrevTime = 20, kStateDtFrame = 21, kStateLen = 22;

        // what k_pairs_hypotheses reads and writes (pairs_hyp.hip): the state and knots as they are, the uploaded times, the
        // options as uploaded; candidate (b, m) at entry b * M + m of cand_t (3N doubles each) and cand_R (4N)
        struct HypArgs
        {
            double *state;                     // B x kStateLen: dt_frame is written
            const double *kt, *kR;             // the knots before the call: B x 3N, B x 4N
            double *cap, *exp, *t0;            // the motion's times, B each: published
            const double *times;               // [cap | exp | t0] as uploaded
            const mbavo_pairs_hyp_opts *opts;
            double *cand_t, *cand_R;
            int B, N;
        };
        // what k_pairs_hyp_select reads and writes: the cost-only evaluation of the B * M entries, the candidates, the knots the
        // problems point at
        struct HypSelectArgs
        {
            const int *counts;                 // B x L
            const double *blocks, *valid;      // entry e: blocks[e * E] its cost, valid[e] its in-bounds pixels
            const double *cand_t, *cand_R;
            double *kt, *kR;
            const mbavo_pairs_hyp_opts *opts;
            mbavo_pairs_hyp *out;              // B
            int B, L, N, E, P;                 // P: the patch size of the options' level
        };

        struct PairCamera; // pairs_prep.h
        // what the depth kernels share (pairs_depth_eval.h: k_pairs_refine, k_pairs_filter, k_pairs_search): the object's table, counts, pattern,
        // motion and camera(s), the tiling and the scratch of the record sums; workgroup e = b * levels + i serves pair b at level
        // (level < 0 ? i : level)
        constexpr int kRefineItems = 1024; // (keypoint, pixel) items of a tile: its keypoints are min(256, kRefineItems / P)
        constexpr int kRefineGroups = 64;  // at most this many workgroups share the tiles of one (pair, level)
        struct DepthEvalArgs
        {
            const PairLevelDesc *desc;         // B x L
            const int *counts;                 // B x L
            const int *pattern;                // level l at pat0[l]
            const double *cap, *exp, *t0;      // B each
            const double *kt, *kR;             // B x 3N, B x 4N
            const PairCamera *of_pair;         // a camera set: B; else null and intr holds the one camera's level-0 intrinsics
            double intr[4];
            double dt, huber_a;
            int L, N, level, levels;           // levels: 1, or L with level == -1
            int S[8], P[8], pat0[8];
            long long out0[8], out_stride;     // first per-keypoint entry of a level within a pair's, entries per pair
            int groups[8];                     // workgroups per (pair, level): min(kRefineGroups, ceil(capacity / tile keypoints)), >= 1
            double *partials;                  // B x levels x kRefineGroups x (the kernel's record sums)
            int *tickets;                      // B x levels, zero between launches
        };
        // k_pairs_refine (pairs_refine.hip): the options as uploaded, the caller's optional per-keypoint arrays, the records
        struct RefineArgs
        {
            DepthEvalArgs ev;
            const mbavo_pairs_refine_opts *opts;
            double *g, *h, *cost;              // or null
            int *valid;                        // or null
            struct mbavo_pairs_refine *out;    // B x levels
        };
        // k_pairs_filter (pairs_filter.hip): the options as uploaded with the B seed words behind them (bit l: seed level l of the
        // pair), the filter state in the layout of level == -1 whatever `level` is, the records
        struct FilterArgs
        {
            DepthEvalArgs ev;
            const mbavo_pairs_filter_opts *opts;
            const int *seed;                   // B
            double *mu, *info;                 // B x st_stride each
            int *n_obs, *n_rej;
            long long st0[8], st_stride;       // first state entry of a level within a pair's, entries per pair
            struct mbavo_pairs_filter *out;    // B x levels
        };
        // k_pairs_search (pairs_search.hip): the options as uploaded, the caller's optional per-keypoint arrays (the refinement's
        // layout; volume: that layout times ND, the candidate fastest), the records
        struct SearchArgs
        {
            DepthEvalArgs ev;
            const mbavo_pairs_search_opts *opts;
            double *rho, *cost_best, *cost_second, *curv, *volume; // or null
            int *best, *num_full;                                  // or null
            struct mbavo_pairs_search *out;    // B x levels
        };
        // k_pairs_photo_fit (pairs_photo.hip): the options as uploaded, the round this launch is (0 .. rounds: the last one forms
        // cost_after alone), the (a, b) the rounds hand on, the records; k_pairs_photo_apply reads the records and the table
        constexpr int kPhotoSums = 7;          // n, Sx, Sy, Sxx, Sxy, C and the count of full keypoints
        struct PhotoArgs
        {
            DepthEvalArgs ev;                  // level >= 0, levels = 1: workgroup row b serves pair b
            const mbavo_pairs_photo_opts *opts;
            int round;
            double *ab;                        // B x 2
            struct mbavo_pairs_photo *out;     // B
        };
        // k_pairs_smooth_index, k_pairs_smooth (pairs_smooth.hip): what the ONE upload of a call holds -- the options, every level's
        // bin edge, then B words (bit l: the index of level l of the pair is rebuilt in this call)
        constexpr int kSmoothBins = 4096;               // at most this many bins per (pair, level)
        constexpr int kSmoothStarts = kSmoothBins + 4;  // ints of a (pair, level)'s bin-start table (bins + 1 used)
        constexpr int kSmoothSums = 7;                  // valid, supported, filled, outliers, moved, support, sum_sq_rel
        struct SmoothXY
        {
            int x, y;
        };
        struct SmoothBlob
        {
            mbavo_pairs_smooth_opts o;
            int s[8];
        };
        // per-slot arrays (perm, pxy, the staging, the filter's state) are in the layout of level == -1 whatever `level` is: pair b
        // from b * st_stride, level l from st0[l]; the caller's arrays in the refinement's (out0, out_stride)
        struct SmoothArgs
        {
            const PairLevelDesc *desc;         // B x L
            const int *counts;                 // B x L
            const SmoothBlob *blob;
            const int *rebuild;                // B
            int L, level, levels;              // levels: 1, or L with level == -1
            int groups[8];                     // gather workgroups per (pair, level): min(kRefineGroups, ceil(capacity / 256)), >= 1
            long long out0[8], out_stride, st0[8], st_stride;
            int *starts;                       // B x L x kSmoothStarts: bin `c` holds perm[starts[c] .. starts[c + 1])
            int *perm;                         // keypoint indices bin after bin, ascending within a bin
            SmoothXY *pxy;                      // their whole-pixel coordinates, in perm's order
            double *stage_D, *stage_rho;       // apply = 1: the depth to write / sync_filter = 1: the mu to write, NaN: none
            const double *info;                // weights = 1: the filter's
            double *mu;                        // sync_filter = 1: the filter's
            const double *weight;              // weights = 2: the caller's
            double *rho;                       // or null
            unsigned char *flags;              // or null
            int *support;                      // or null
            double *partials;                  // B x levels x kRefineGroups x kSmoothSums
            int *tickets;                      // B x levels, zero between launches
            struct mbavo_pairs_smooth *out;    // B x levels
        };
        // k_pairs_carry_warp, k_pairs_carry_index, k_pairs_carry_adopt (pairs_carry.hip): what the ONE upload of a call holds -- the
        // options, then one CarryPair per listed pair (an adopt reads `pair` and `radius` of it alone)
        constexpr int kCarrySaveSums = 3;               // valid, carried, sum_w
        constexpr int kCarryAdoptSums = 4;              // adopted, empty, sum_info, sum_sq_rel
        struct CarryPair
        {
            int pair, radius;                  // the pair's index; the radius its carried set is (being) armed with
            double t[3], R[9];                 // X_old = R X_new + t, R row-major (pixel_math.h: rotation_entries, formed on the host)
        };
        // the carried set and the per-slot arrays are in the layout of level == -1: pair b from b * st_stride, level l from st0[l];
        // workgroup (row) e = i * L + l serves listed pair i at level l
        struct CarryArgs
        {
            const PairLevelDesc *desc;         // B x L
            const int *counts;                 // B x L
            const PairCamera *of_pair;         // a camera set: B; else null and intr holds the one camera's level-0 intrinsics
            double intr[4];
            const void *opts;                  // mbavo_pairs_carry_save_opts / mbavo_pairs_carry_adopt_opts as uploaded
            const CarryPair *list;             // n, behind the options
            int L;
            int groups[8];                     // warp / adopt workgroups per (pair, level): min(kRefineGroups, ceil(capacity / 256)), >= 1
            long long st0[8], st_stride;
            int *starts;                       // B x L x kSmoothStarts: bin `c` holds perm[starts[c] .. starts[c + 1]); entry nb: the total
            int *perm;                         // source keypoint indices of the carried points bin after bin, ascending within a bin
            SmoothXY *pxy;                     // their pixels in the new keyframe, in perm's order
            SmoothXY *sxy;                     // by source index: the staged pixel, x < 0: not carried
            double *c_rho, *c_w;               // by source index: rho' and w' of a carried point
            const double *info_in;             // save, weights = 1: the filter's info
            double *mu, *info;                 // adopt, seed_filter = 1: the filter's state
            int *n_obs, *n_rej;
            double *rho;                       // adopt: the caller's arrays, or null
            double *info_out;
            int *count;
            unsigned char *flags;
            double *partials;                  // B x L x kRefineGroups x (the kernel's sums)
            int *tickets;                      // B x L, zero between launches
            void *out;                         // n x L records of the call
        };

        // k_pairs_prune (pairs_prune.hip): what the ONE upload of a call holds -- the options, then the n listed pair indices; workgroup
        // e = i * levels + j serves listed pair i at level (level < 0 ? j : level).  The filter's state is in the layout of level ==
        // -1 whatever `level` is, the caller's two byte arrays in the refinement's (out0, out_stride)
        struct PruneArgs
        {
            const PairLevelDesc *desc;         // B x L
            int *counts;                       // B x L: a pruned (pair, level)'s count is written
            const mbavo_pairs_prune_opts *opts;
            const int *list;                   // n, behind the options
            int L, level, levels;              // levels: 1, or L with level == -1
            long long out0[8], out_stride, st0[8], st_stride;
            double *mu, *info;                 // the filter's state, moved along; null: it does not exist yet
            int *n_obs, *n_rej;
            const unsigned char *flags;        // or null
            unsigned char *keep;               // or null
            struct mbavo_pairs_prune *out;     // n x levels records of the call
            int *new_counts;                   // B x L behind the records: entry b * L + l of a served (pair, level), its count after the call
        };

#if defined(__HIPCC__)
        template <int KDEG>
        __device__ bool spline_pose(const double *__restrict__ kt, const double *__restrict__ kR, int N, double t0, double dt, double t, Quat &q, double p[3])
        { // SplineSE3::GetPose without Jacobians
            int idx;
            double u;
            if (!spline_segment_checked(t, t0, dt, N, KDEG, idx, u)) return false; // (a NaN or infinite time included)
            double c[KDEG];
            trans_coeffs<KDEG>(u, c);
            spline_translation<KDEG>(kt + 3 * idx, c, p);
            q = spline_rotation<KDEG, false>(kR + 4 * idx, u, nullptr);
            return true;
        }
#endif
    }
} // namespace mbavo

#endif
