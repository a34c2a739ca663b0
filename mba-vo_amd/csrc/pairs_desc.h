// pairs_desc.h -- what the two halves of a batch of keyframe pairs share on the device (pairs_prep.hip: the images and keypoints;
// pairs_track.hip: the tracker): one (pair, level) of the device-resident table and the alignment of the arena's arrays.
#ifndef MBAVO_PAIRS_DESC_H
#define MBAVO_PAIRS_DESC_H

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
    }
} // namespace mbavo

#endif
