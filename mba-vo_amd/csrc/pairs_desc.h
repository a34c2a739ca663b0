// pairs_desc.h -- what the parts of a batch of keyframe pairs share on the device (pairs_prep.hip: the images and keypoints;
// pairs_track.hip: the tracker; pairs_report.hip: the report): one (pair, level) of the device-resident table, the alignment of the
// arena's arrays, the report kernel's arguments and the spline sample that tracker and report both take at the capture time.
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

    namespace pairs
    {
        constexpr long long kAlign = 256;
        inline long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

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

#if defined(__HIPCC__)
        template <int KDEG>
        __device__ bool spline_pose(const double *__restrict__ kt, const double *__restrict__ kR, int N, double t0, double dt, double t, Quat &q, double p[3])
        { // SplineSE3::GetPose without Jacobians
            int idx;
            double u;
            spline_segment(t, t0, dt, idx, u);
            if (!(t == t) || idx < 0 || idx + KDEG > N) return false;
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
