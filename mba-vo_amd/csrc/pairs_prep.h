// pairs_prep.h -- the input side of a batch of keyframe pairs (include/mbavo.h: mbavo_pairs_*): pyramids, keyframe gradient
// images and semi-dense keypoints of B pairs x L levels in a constant number of launches, laid out as the B x L mbavo_problem
// array mbavo_lm_batch_levels takes, and the tracker state that carries them from frame to frame.  The image side (create, prepare,
// update, the motion) is in pairs_prep.hip, the tracker (assess, states, predict, commit) in pairs_track.hip, the report in
// pairs_report.hip, the motion hypotheses in pairs_hyp.hip; all find the arrays through one layout value, PairsArena.
//
// The depth stages -- refinement (pairs_refine.hip), filter (pairs_filter.hip), search (pairs_search.hip), smoothing
// (pairs_smooth.hip), the hand-over to the next keyframe (pairs_carry.hip), the pruning (pairs_prune.hip) -- and the brightness
// match on the same evaluation (pairs_photo.hip) are a policy, an options check and an argument block
// each; what surrounds their launches is here ONCE: DepthCall (a call's scratch, mirror, event and statistics), DepthSlots (the
// per-keypoint slot layout and the workgroups per (pair, level), computed in create), filter_arrays, the options checks.
#ifndef MBAVO_PAIRS_PREP_H
#define MBAVO_PAIRS_PREP_H

#include "../../include/mbavo.h"
#include "engine.h"
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <vector>

namespace mbavo
{
    // Everything create allocates, as offsets into ONE device allocation (every array 256-byte aligned).  Pure host arithmetic:
    // mbavo_pairs_plan reports it without a device.
    struct PairsPlan
    {
        int B, L, format, grad_bytes;          // grad_bytes per pixel: 8 (float pairs) or 4 (half pairs / packed words)
        int H[8], W[8];
        int ch[8], cw[8], cells_w[8], cells[8]; // grid of FeatureDetectorBase.cpp:56-64
        int cell0[9];                           // first cell of every level within a pair's picks
        int dense;                              // mbavo_pairs_opts.every_candidate: no grid, no picks; cells .. cell0 stay 0
        int cap[8];                             // keypoint capacity of every level: its cells, or (every candidate) its H * W pixels
        int seg0[9];                            // every candidate: first segment count (one per 256 pixels) of every level within a pair's
        long long px0[9];                       // first pixel of every level within an image (levels padded to 16 pixels)
        long long kp0[9];                       // first double of every level within a pair's keypoint slice ([xy 2 cap | z cap], cap even)
        int pat0[9];                            // first int of every level's pattern
        long long img_stride, grad_stride, kp_stride; // bytes per image / per pair's gradients, doubles per pair's keypoints
        int N;
        // mbavo_pairs_opts.valid_radius > 0: one clearance pyramid per map behind off_clear, clear_stride bytes each, level l at
        // clear0[l] within it (every level 256-byte aligned); else nothing
        long long clear0[9], clear_stride;
        // mbavo_pairs_opts.mask = 1: one stored level-0 mask per camera behind off_mask, mask_stride bytes each, and the clearance
        // pyramids above whatever valid_radius is; else nothing
        long long mask_stride;
        // byte offsets of the arrays (off_map: mbavo_pairs_opts.undistort != 0: the level-0 undistortion map, 8 H W bytes, or with
        // mbavo_pairs_opts.num_cameras = G the G maps one behind the other; else nothing)
        long long off_img, off_grad, off_kp, off_picks, off_seg, off_counts, off_desc, off_cur_ptrs, off_pattern, off_map, off_clear, off_mask, off_motion, total;
    };
    // MBAVO_E_ARG as mbavo_pairs_create returns it, 0 and a filled plan otherwise
    int pairs_plan(const mbavo_pairs_opts *o, PairsPlan &plan);

    struct DepthConv;     // keyframe_math.h: the constants of the depth formats
    struct MapCamera;     // camera_math.h: a camera of a set as the map kernel reads it
    struct PairLevelDesc; // pairs_desc.h: one (pair, level) of the device table
    struct CellPick;      // vo_frontend.h
    namespace pairs
    {
        // mbavo_pairs_opts.num_cameras > 0: what the kernels read of pair b's camera -- the level-0 intrinsics of its undistorted
        // images and the camera's place among the maps -- and where they find it (by value in the kernels' arguments)
        struct PairCamera
        {
            double fx, fy, cx, cy;
            int cam, pad;
        };
        struct CameraSet
        {
            const PairCamera *of_pair; // B
            const float *maps;         // undistort != 0: G maps of map_floats = 2 H0 W0 floats each
            long long map_floats;
            int Hs, Ws;                // the raw size, of every camera
            float unit, max;           // DepthConv's, from the options
        };
        // mbavo_pairs_opts.valid_radius > 0 with a camera set: the G clearance pyramids, `stride` bytes each
        struct ClearSet
        {
            const unsigned char *base;
            long long stride;
        };
        // where a refresh takes the keypoints of its keyframes from: the depth maps the detector looks its picks up in (row y: the map
        // of grid row y), or -- points set -- the caller's level-0 points (row y: entries offsets[y] .. offsets[y + 1] - 1 of xy and
        // z; the offsets come on the host and travel into the context's scratch)
        struct KeypointSource
        {
            const void *d_depth = nullptr;
            bool points = false;
            const int *h_offsets = nullptr, *d_offsets = nullptr;
            const double *d_xy = nullptr, *d_z = nullptr;
        };
        struct ScoreSlices; // pairs_desc.h
        struct AssessArgs; // pairs_track.hip: the kernels' argument blocks
        struct TrackArgs;
        struct DepthEvalArgs; // pairs_desc.h
        struct CarryArgs;
        // what one call cost: kernel launches, stream synchronisations, bytes read back from the device
        struct CallStats
        {
            long long launches = 0, syncs = 0, bytes_back = 0;
            void get(long long out[3]) const { out[0] = launches; out[1] = syncs; out[2] = bytes_back; }
        };
        // the launches of the evaluation the engine just enqueued, from its own witnesses (pairs_report.hip; include/mbavo.h:
        // mbavo_pairs_report_stats)
        long long evaluation_launches(Engine &eng);
    }

    // The layout of the object's ONE device allocation, built once in create: the plan's arrays (the motion behind off_motion is
    // [cap B | exp B | knots_t B x 3N | knots_R B x 4N]) and, behind plan.total, what mbavo_pairs_plan does not report -- [t0 B |
    // state B x kStateLen | predict's times | frames B] and with num_cameras = G what set_cameras uploads in one copy, [MapCamera G |
    // PairCamera B] (every array 256-byte aligned).  The typed pointers take a base; nothing else adds an offset to the arena.
    struct PairsArena
    {
        PairsPlan plan{};
        long long o_exp = 0, o_knots_t = 0, o_knots_R = 0, o_t0 = 0, o_state = 0, o_times = 0, o_frames = 0, o_map_cams = 0, o_pair_cams = 0;
        long long cams_bytes = 0, bytes = 0; // of [MapCamera G | PairCamera B] (num_cameras = 0: nothing), of the allocation
        // [knots_t | knots_R | pad | t0 | state] moves in ONE copy (set_states, get_states): its start and its length.  The pointers
        // of these four also take its pinned mirror, which starts `from` = span_first bytes into the layout.
        long long span_first = 0, span_bytes = 0;
        PairsArena() = default;
        PairsArena(const PairsPlan &p, int num_cameras); // pairs_prep.hip
        unsigned char *images(char *b) const { return (unsigned char *)(b + plan.off_img); } // [keyframes B | current frames B] x img_stride
        char *grad(char *b) const { return b + plan.off_grad; }                               // B x grad_stride
        double *keypoints(char *b) const { return (double *)(b + plan.off_kp); }              // B x kp_stride doubles
        CellPick *picks(char *b) const { return (CellPick *)(b + plan.off_picks); }           // grid selection: B x cell0[L]
        int *seg(char *b) const { return (int *)(b + plan.off_seg); }                         // every candidate: B x seg0[L]
        int *counts(char *b) const { return (int *)(b + plan.off_counts); }                   // B x L
        PairLevelDesc *desc(char *b) const { return (PairLevelDesc *)(b + plan.off_desc); }   // B x L
        const unsigned char **cur_ptrs(char *b) const { return (const unsigned char **)(b + plan.off_cur_ptrs); } // B x L
        int *pattern(char *b) const { return (int *)(b + plan.off_pattern); }                 // level l at pat0[l]
        float *maps(char *b) const { return (float *)(b + plan.off_map); }                    // undistort != 0: G' maps of 2 H0 W0 floats
        unsigned char *clear(char *b) const { return (unsigned char *)(b + plan.off_clear); } // G' pyramids of clear_stride bytes
        unsigned char *masks(char *b) const { return (unsigned char *)(b + plan.off_mask); }  // mask = 1: G' masks of mask_stride bytes
        double *cap(char *b) const { return (double *)(b + plan.off_motion); }                // B; the motion starts here
        double *exp(char *b) const { return (double *)(b + o_exp); }                          // B
        double *knots_t(char *b, long long from = 0) const { return (double *)(b + (o_knots_t - from)); } // B x 3N
        double *knots_R(char *b, long long from = 0) const { return (double *)(b + (o_knots_R - from)); } // B x 4N
        double *t0(char *b, long long from = 0) const { return (double *)(b + (o_t0 - from)); }           // B
        double *state(char *b, long long from = 0) const { return (double *)(b + (o_state - from)); }     // B x kStateLen
        double *times(char *b) const { return (double *)(b + o_times); }                      // [cap | exp | t0] as a predict uploads them
        mbavo_pairs_frame *frames(char *b) const { return (mbavo_pairs_frame *)(b + o_frames); } // B
        // G and B (also within a host copy of the two, which starts `from` = o_map_cams bytes into the layout)
        MapCamera *map_cameras(char *b, long long from = 0) const { return (MapCamera *)(b + (o_map_cams - from)); }
        pairs::PairCamera *pair_cameras(char *b, long long from = 0) const { return (pairs::PairCamera *)(b + (o_pair_cams - from)); }
    };

    // A device or pinned host allocation that frees itself (move-only).  Its owner selects the device before it lets go of one.
    template <class T, bool PINNED>
    struct HipArray
    {
        T *p = nullptr;
        HipArray() = default;
        HipArray(HipArray &&o) noexcept { std::swap(p, o.p); }
        HipArray &operator=(HipArray &&o) noexcept { std::swap(p, o.p); return *this; }
        ~HipArray() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); }
        hipError_t alloc(size_t bytes) // (of an empty array)
        {
            const hipError_t e = PINNED ? hipHostMalloc((void **)&p, bytes) : hipMalloc((void **)&p, bytes);
            return e == hipSuccess ? e : (p = nullptr, e);
        }
        operator T *() const { return p; }
    };
    template <class T> using DeviceArray = HipArray<T, false>;
    template <class T> using PinnedArray = HipArray<T, true>;

    class PairBatch;
    namespace pairs
    {
        // The per-keypoint slots of the depth stages' own arrays (the filter's state, the spatial indices, the staging) and of the
        // caller's per-keypoint arrays at level = -1: pair b from b * st_stride, level l from st0[l] (st0[L] = st_stride), n_slots =
        // B * st_stride in all.  Pure host arithmetic on the plan, done once in create.
        struct DepthSlots
        {
            long long st0[9] = {}, st_stride = 0;
            size_t n_slots = 0;
            int groups256[8] = {}; // workgroups per (pair, level) of a kernel that takes 256 keypoints per tile (smoothing, hand-over)
            DepthSlots() = default;
            explicit DepthSlots(const PairsPlan &p);
            // min(kRefineGroups, ceil(cap / T)), >= 1: the workgroups that share the tiles of T keypoints of one (pair, level)
            static int groups(long long cap, int T);
            // the caller's per-keypoint arrays of a call on `level`: every level's first entry into out0; returns the entries per pair
            long long outs(int level, long long out0[8]) const;
            // the grid's width of a call on `level` (-1: every level): the most of g's workgroups over the levels it reports
            static int width(int level, const int g[8]);
        };

        // The scratch of ONE depth stage of `pb`, allocated at the stage's first call (not part of the plan): device [records B x L
        // | the workgroups' partial sums B x L x 64 x sums | tickets B x L | options] and a pinned mirror [records | options], with
        // the event that says the last upload has left the mirror, and what the stage's last call cost.  It destroys its own event
        // and its arrays free themselves, once the owner has selected the device and waited for the stream.
        struct DepthCall
        {
            PairBatch &pb;
            DeviceArray<char> dev;
            PinnedArray<char> mirror;
            hipEvent_t copied = nullptr;
            char *records = nullptr, *d_opts = nullptr, *h_opts = nullptr; // where open put them: on the device, h_opts in the mirror
            double *partials = nullptr;
            int *tickets = nullptr;
            CallStats stats;
            explicit DepthCall(PairBatch &owner) : pb(owner) {}
            ~DepthCall() { if (copied) (void)hipEventDestroy(copied); }
            // both allocations at the first use (the tickets zeroed; the sizes are the same at every call); from the second call on
            // the wait for the upload `copied` marks -- a call that read nothing back may still be reading the mirror
            // (levels: the records, sums and tickets per pair; 0: the object's L)
            hipError_t open(size_t rec_bytes_max, int sums, size_t opt_bytes, int levels = 0);
            // the ONE copy of `bytes` of the options to the device, and `copied` behind it
            hipError_t upload(size_t bytes);
            // the end of a call: the launch error (h_out null: nothing is waited for) or PairBatch::read_back, counted in `st` or stats
            int finish(void *h_out, size_t rec_bytes, CallStats *st = nullptr);
        };

        // The scratch of mbavo_pairs_match_brightness as typed pointers into its opened DepthCall (one record, one ticket and one
        // set of sums per pair): the B x 2 doubles of (a, b) the rounds hand on lie behind the options, which fill whole doubles
        struct PhotoScratch
        {
            const DepthCall &call;
            static size_t opt_bytes(int B) { return sizeof(mbavo_pairs_photo_opts) + sizeof(double) * 2 * (size_t)B; }
            struct mbavo_pairs_photo *records() const { return (struct mbavo_pairs_photo *)call.records; }
            const mbavo_pairs_photo_opts *opts() const { return (const mbavo_pairs_photo_opts *)call.d_opts; }
            double *ab() const { return (double *)(call.d_opts + sizeof(mbavo_pairs_photo_opts)); }
        };
        static_assert(sizeof(mbavo_pairs_photo_opts) % sizeof(double) == 0, "(a, b) behind the options: aligned doubles");

        // The photometric calibration of the arriving images (include/mbavo.h: mbavo_pairs_set_photometric; pairs_photocal.hip),
        // allocated at the first call and kept (not part of the plan): the n tables of 256 floats with their pinned mirror; the n
        // inverse vignettes of Hr x Wr floats once a call brought a vignette.  `active`: level 0 of every intake goes through the
        // calibrated kernels.  Its arrays free themselves, once the owner has selected the device and waited for the stream.
        struct PhotoCal
        {
            DeviceArray<float> luts, inv;
            PinnedArray<float> mirror;
            bool active = false, vignette = false;
            bool lds = true;        // the table of a grid row's calibration is staged in LDS (MBAVO_PAIRS_PHOTOCAL_LDS=0: plain loads)
            int Hr = 0, Wr = 0;     // the geometry of the inverse vignettes as allocated: the raw camera's, or the object's H0 x W0
            CallStats stats;
        };

        // The keypoint response of the detector calls (include/mbavo.h: mbavo_pairs_set_detector; pairs_score.hip).  The score
        // slices are allocated at the first call that asks for the corner score and kept (not part of the plan): one float per pixel
        // of every keyframe level, laid out as the gradient slices are.  They free themselves, once the owner has selected the device
        // and waited for the stream.
        struct Detector
        {
            int score = 0, radius = 0; // 0: gradient magnitude, the object as created
            float threshold = 0.f;     // score = 1: what a candidate must exceed (the creation threshold is not read)
            DeviceArray<float> slices;
            long long bytes = 0;
        };

        // the options checks of the depth stages (a failed one has touched nothing)
        inline bool bad_limit(double v) { return !std::isfinite(v) || v < 0.0; }
        inline bool flags01(std::initializer_list<int> f) { return std::all_of(f.begin(), f.end(), [](int v) { return v == 0 || v == 1; }); }
        // the depth limits: finite and >= 0, z_min = 0 means 1e-2, a z_max that is set is not below z_min
        inline int depth_limits(double &z_min, double z_max)
        {
            if (bad_limit(z_min) || bad_limit(z_max)) return MBAVO_E_ARG;
            if (z_min == 0.0) z_min = 1e-2;
            return z_max != 0.0 && z_max < z_min ? MBAVO_E_ARG : 0;
        }
    }

    class PairBatch
    {
    public:
        PairBatch(Engine &eng) : eng_(eng) {}
        ~PairBatch();
        PairBatch(const PairBatch &) = delete;
        PairBatch &operator=(const PairBatch &) = delete;
        int create(const mbavo_pairs_opts *o);
        // (d_depth: the maps in the format of mbavo_pairs_opts.depth_format -- float z, float ray distance or uint16)
        int prepare(const unsigned char *d_sharp, const void *d_depth, const unsigned char *d_blur, int *h_counts);
        // keypoints from the caller in place of the detector (include/mbavo.h: mbavo_pairs_prepare_points, _update_points): row i of
        // the host offsets lists the level-0 points of pair i (prepare) or of the i-th listed pair (update)
        int prepare_points(const unsigned char *d_sharp, const unsigned char *d_blur, const int *h_offsets, const double *d_xy, const double *d_z,
                           int *h_counts);
        int update_points(const unsigned char *d_blur, int n_key, const int *h_key_pairs, const unsigned char *d_sharp, const int *h_offsets,
                          const double *d_xy, const double *d_z, int *h_counts);
        // mbavo_pairs_opts.undistort != 0: the camera of the raw images; one launch that fills the object's undistortion map
        int set_camera(const mbavo_camera_radtan *from);
        int set_camera(const mbavo_camera_unified *from); // (the same map, filled for a unified camera; the last call decides)
        // mbavo_pairs_opts.num_cameras = G: the G cameras and every pair's index; one copy, one launch that fills the G maps
        int set_cameras(int G, const mbavo_pairs_camera *h_cams, const int *h_camera_of_pair);
        // mbavo_pairs_opts.mask = 1: the masks of all cameras (geometry 0: undistorted, copied; 1: raw, warped through the maps in one
        // launch), then the clearance pyramids again
        int set_masks(int geometry, int n, const unsigned char *d_masks);
        // the geometry of the points of later prepare_points / update_points calls: 0 the object's undistorted one, 1 the raw camera's
        // (undistort != 0), inverted inside the points kernel (include/mbavo.h: mbavo_pairs_set_points_geometry)
        int set_points_geometry(int geometry);
        int set_motion(const double *h_cap, const double *h_exp, const double *h_t0, double dt, const double *h_knots_t, const double *h_knots_R);
        int get_knots(double *h_knots_t, double *h_knots_R);
        const mbavo_problem *problems() const { return probs_.data(); }
        int count() const { return (int)probs_.size(); }
        void last_stats(long long out[4]) const;
        // the step from frame to frame (include/mbavo.h: mbavo_pairs_update, mbavo_pairs_assess)
        int update(const unsigned char *d_blur, int n_key, const int *h_key_pairs, const unsigned char *d_sharp, const void *d_depth, int *h_counts);
        int assess(double flow_mag0, double flow_mag1, double max_blur_kernel_mag, mbavo_pairs_assessment *h_out);
        void update_stats(long long out[3]) const { upd_stats_.get(out); }
        void assess_stats(long long out[3]) const { ass_stats_.get(out); }
        // tracker state on the device (include/mbavo.h: mbavo_pairs_set_states .. mbavo_pairs_commit)
        int set_states(const mbavo_vo_state *h_states);
        int get_states(mbavo_vo_state *h_states);
        int predict(const double *h_cap, const double *h_exp);
        int commit(double flow_mag0, double flow_mag1, double max_blur_kernel_mag, mbavo_pairs_frame *h_out);
        void track_stats(long long out[6]) const { pre_stats_.get(out); com_stats_.get(out + 3); }
        // every pair's pose information, covariance and keypoint flags at its knots as they are (include/mbavo.h: mbavo_pairs_report)
        int report(double max_chi_square_error, struct mbavo_pairs_report *h_out, double *d_patch_cost, unsigned char *d_flags);
        void report_stats(long long out[3]) const { rep_stats_.get(out); }
        // predict with every pair's start picked among M motion hypotheses (include/mbavo.h: mbavo_pairs_predict_hypotheses)
        int predict_hypotheses(const double *h_cap, const double *h_exp, const mbavo_pairs_hyp_opts *o, mbavo_pairs_hyp *h_out);
        void hyp_stats(long long out[3]) const { hyp_stats_.get(out); }
        // every keypoint's depth gradient, curvature and damped inverse-depth step (include/mbavo.h: mbavo_pairs_refine_depths)
        int refine_depths(const mbavo_pairs_refine_opts *o, struct mbavo_pairs_refine *h_out, double *d_g, double *d_h, double *d_cost, int *d_valid);
        void refine_stats(long long out[3]) const { refine_call_.stats.get(out); }
        // the recursive inverse-depth filter over the frames of a keyframe (include/mbavo.h: mbavo_pairs_filter_depths, _filter_state)
        int filter_depths(const mbavo_pairs_filter_opts *o, struct mbavo_pairs_filter *h_out);
        int filter_state(double **d_mu, double **d_info, int **d_n_obs, int **d_n_rej, long long *h_pair_stride, long long h_level_offset[8]) const;
        void filter_stats(long long out[3]) const { filter_call_.stats.get(out); }
        // every keypoint's depth searched among ND candidates (include/mbavo.h: mbavo_pairs_search_depths)
        int search_depths(const mbavo_pairs_search_opts *o, struct mbavo_pairs_search *h_out, double *d_rho, double *d_cost_best, double *d_cost_second,
                          double *d_curv, int *d_best, int *d_num_full, double *d_volume);
        void search_stats(long long out[3]) const { search_call_.stats.get(out); }
        // every keypoint's depth smoothed over its image neighbours (include/mbavo.h: mbavo_pairs_smooth_depths)
        int smooth_depths(const mbavo_pairs_smooth_opts *o, struct mbavo_pairs_smooth *h_out, const double *d_weight, double *d_rho,
                          unsigned char *d_flags, int *d_support);
        void smooth_stats(long long out[3]) const { smooth_call_.stats.get(out); }
        // a keyframe's keypoint depths handed to the pair's next keyframe (include/mbavo.h: mbavo_pairs_carry_save, _carry_adopt)
        int carry_save(int n, const int *h_pairs, const double *h_T, const mbavo_pairs_carry_save_opts *o, struct mbavo_pairs_carry_save *h_out);
        int carry_adopt(int n, const int *h_pairs, const mbavo_pairs_carry_adopt_opts *o, struct mbavo_pairs_carry_adopt *h_out, double *d_rho,
                        double *d_info, int *d_count, unsigned char *d_flags);
        void carry_save_stats(long long out[3]) const { csv_stats_.get(out); }
        void carry_adopt_stats(long long out[3]) const { cad_stats_.get(out); }
        // flagged keypoints removed from the object's own arrays, depths and filter state moved along (include/mbavo.h:
        // mbavo_pairs_prune_keypoints); n = 0 with a null list: every pair
        int prune_keypoints(int n, const int *h_pairs, const mbavo_pairs_prune_opts *o, const unsigned char *d_flags, struct mbavo_pairs_prune *h_out,
                            unsigned char *d_keep);
        void prune_stats(long long out[3]) const { prune_call_.stats.get(out); }
        // every pair's brightness gain and offset against its keyframe, fitted and optionally removed from its current frame
        // (include/mbavo.h: mbavo_pairs_match_brightness)
        int match_brightness(const mbavo_pairs_photo_opts *o, struct mbavo_pairs_photo *h_out);
        void photo_stats(long long out[3]) const { photo_call_.stats.get(out); }
        // the sensor's inverse response and vignette, applied where level 0 is taken in (include/mbavo.h: mbavo_pairs_set_photometric)
        int set_photometric(int n, const double *h_G, const float *d_vignette, const mbavo_pairs_photocal_opts *o);
        int clear_photometric();
        void photocal_stats(long long out[3]) const { photocal_.stats.get(out); }
        // the response later prepares, updates and track_frames select keypoints by (include/mbavo.h: mbavo_pairs_set_detector)
        int set_detector(const mbavo_pairs_detector_opts *o);
        void detector_stats(long long out[3]) const { out[0] = detector_.score; out[1] = detector_.radius; out[2] = detector_.bytes; }
        int pairs() const { return plan_.B; }
        int levels() const { return plan_.L; }

    private:
        // set_camera for either camera struct: one launch of its map function into the object's map
        template <class Camera>
        int set_camera_with(const Camera *from, int (*fill_map)(Engine &, const Camera *, const double *, int, int, float *));
        // level 0 of the images that changed into the object's own storage (rows as in refresh).  undistort != 0: remapped from
        // the raw images in ONE launch; else one strided copy per image array, the keyframes of a list through one launch
        int level0(int n_key, const int *d_keys, const unsigned char *d_sharp, int n_cur, const unsigned char *d_blur, pairs::CallStats &s);
        // the same under a photometric calibration (pairs_photocal.hip): ONE launch either way -- the calibrated remap, or with
        // undistort = 0 the calibrated copy of all n_key + n_cur images in place of the copies and the scatter
        int level0_calibrated(int n_key, const int *d_keys, const unsigned char *d_sharp, int n_cur, const unsigned char *d_blur, pairs::CallStats &s);
        // level 0 and the pyramids below it of the images that changed (n_key keyframes: rows of d_keys, or pairs 0 .. n_key - 1
        // where it is null -- a prepare; then n_cur current frames), gradients and keypoints of those keyframes (from `src`: the
        // detector on row y's depth map, or row y's points), the counts read back into probs_[i].K, one synchronisation
        int refresh(int n_key, const int *d_keys, const unsigned char *d_sharp, int n_cur, const unsigned char *d_blur,
                    const pairs::KeypointSource &src, pairs::CallStats &s);
        // score = 1: the corner scores of every level of n_key keyframes (rows of d_keys, or pairs 0 .. n_key - 1 where it is null)
        // into the object's score slices, ONE launch, counted in s (pairs_score.hip); score_slices: where the kernels find them
        void score_levels(int n_key, const int *d_keys, pairs::CallStats &s);
        pairs::ScoreSlices score_slices() const;
        // levels 1 .. L-1 below level 0 as it is, of n_key keyframes (rows of d_keys, or pairs 0 .. n_key - 1 where it is null) and
        // then of the first n_cur pairs' current frames: ceil((L - 1) / 3) launches, counted in s
        void pyramids(int n_key, const int *d_keys, int n_cur, pairs::CallStats &s);
        // what prepare and prepare_points, update and update_points share: the checks, the offsets' upload, the refresh
        int prepare_from(const unsigned char *d_sharp, const unsigned char *d_blur, pairs::KeypointSource src, int *h_counts);
        int update_from(const unsigned char *d_blur, int n_key, const int *h_key_pairs, const unsigned char *d_sharp, pairs::KeypointSource src,
                        int *h_counts);
        // the host checks of a points call on `rows` lists (MBAVO_E_ARG, MBAVO_E_RANGE: include/mbavo.h), nothing touched
        int check_points(int rows, const int *h_offsets, const double *d_xy, const double *d_z) const;
        // the rows + 1 offsets into the context's scratch, ONE copy on the stream; null: the scratch could not be had
        const int *upload_offsets(int rows, const int *h_offsets);
        // f(the camera policy of the keypoint kernels: pairs_prep.hip, OneCamera / PairCameras)
        template <class F>
        int with_camera(F &&f) const;
        // f(the policy of the points kernel: `cam` itself, or with points_geometry_ = 1 RawPoints around it)
        template <class CAM, class F>
        int with_points_geometry(const CAM &cam, F &&f) const;
        // every blur sample of every level of every pair on knots that exist (h_t0 null: a frame starts at cap - exp / 2)
        bool samples_on_knots(const double *h_cap, const double *h_exp, const double *h_t0, double dt) const;
        void publish_times(const double *h_cap, const double *h_t0, double dt); // start_idx_, t0 and dt of probs_
        hipError_t upload_times(const double *h_cap, const double *h_exp); // [cap | exp | cap - exp / 2] into the arena, ONE copy
        // the end of a call: the launch error, `bytes` (0: nothing) from d_src into the pinned h_mirror, ONE synchronisation, on to
        // h_out where it is set; s gets the synchronisation and the bytes (the launches are the call's to count)
        int read_back(const void *d_src, void *h_mirror, void *h_out, size_t bytes, pairs::CallStats &s);
        // what refine_depths and filter_depths share (pairs_refine.hip): the build's limits on the reported levels (MBAVO_E_ARG), the
        // evaluation's arguments but for the record scratch, the grid's width, the dynamic LDS
        int depth_eval_args(int level, pairs::DepthEvalArgs &a, int &width, size_t &lds) const;
        friend struct pairs::DepthCall; // (the stream, B x L, read_back)
        // the filter's state, each array in DepthSlots' layout: [mu | info | n_obs | n_rej] of filter_state_
        struct FilterArrays
        {
            double *mu, *info;
            int *n_obs, *n_rej;
        };
        FilterArrays filter_arrays() const
        {
            double *mu = (double *)filter_state_.p, *info = mu + slots_.n_slots;
            int *n_obs = (int *)(info + slots_.n_slots);
            return FilterArrays{mu, info, n_obs, n_obs + slots_.n_slots};
        }
        // what carry_save and carry_adopt share (pairs_carry.hip): the checks of the list (MBAVO_E_ARG); the kernels' arguments but
        // for the caller's arrays, the carried sets (allocated at the first call), the opened scratch with the list behind
        // opts_size bytes of options
        int carry_list(int n, const int *h_pairs) const;
        int carry_args(pairs::CarryArgs &a, size_t opts_size);
        pairs::AssessArgs assess_args(double flow_mag0, double flow_mag1, double max_blur_kernel_mag) const;
        pairs::TrackArgs track_args() const;
        DepthConv depth_conv() const; // level-0 intrinsics, depth_unit, depth_max of the options
        bool camera_missing() const;  // a prepare or an update cannot run yet: no set_camera / set_cameras so far
        // a camera call may bring raw images of Hs x Ws: any size until inverse vignettes were made for one (mbavo_pairs_set_photometric)
        bool raw_size_fixed(int Hs, int Ws) const { return opts_.undistort != 0 && photocal_.inv && (Hs != photocal_.Hr || Ws != photocal_.Wr); }
        pairs::CameraSet camera_set() const; // num_cameras > 0: where the kernels find a pair's camera
        // valid_radius > 0 or mask = 1: the clearance pyramids of the n cameras from the maps just enqueued (undistort = 0: none) and
        // the stored masks (mask = 0: none) (include/mbavo.h: 3 or 4 launches, with radius 0 two fewer; nothing waited for)
        int fill_clearance(int n);
        bool has_clearance() const { return opts_.valid_radius > 0 || opts_.mask != 0; }
        int cameras() const { return opts_.num_cameras > 0 ? opts_.num_cameras : 1; } // G': maps, masks and pyramids the object holds
        Engine &eng_;
        PairsArena lay_;                       // where everything is in arena_
        const PairsPlan &plan_ = lay_.plan;
        mbavo_pairs_opts opts_{};
        // every buffer frees itself, after the destructor has selected the device and waited for the stream
        DeviceArray<char> arena_;
        PinnedArray<int> h_counts_;    // B x L
        PinnedArray<double> h_motion_; // staging of [cap B | exp B | knots_t B x 3N | knots_R B x 4N | t0 B]
        // the step's own small buffers (not part of the plan): device [assessments B | key list B ints], pinned mirrors
        DeviceArray<char> step_;
        PinnedArray<char> h_state_;    // mirror of the arena's [knots_t .. state] (PairsArena::span_first)
        PinnedArray<double> h_times_;  // [cap | exp | t0]
        PinnedArray<mbavo_pairs_frame> h_frames_;
        bool states_set_ = false, pending_ = false;
        double state_dt_ = 0;
        pairs::CallStats pre_stats_, com_stats_;
        PinnedArray<mbavo_pairs_assessment> h_assess_;
        PinnedArray<int> h_keys_;
        bool prepared_ = false, motion_set_ = false;
        int raw_H_ = 0, raw_W_ = 0; // the raw camera's image size (set_camera, set_cameras); 0: no camera yet
        mbavo_pairs_camera raw_cam_{}; // num_cameras == 0: the raw camera as set_camera took it, with opts_.intrinsics as its `to`
        int points_geometry_ = 0;      // mbavo_pairs_set_points_geometry
        bool cameras_set_ = false;  // num_cameras > 0: set_cameras has run
        PinnedArray<char> h_cams_;  // mirror of [MapCamera G | PairCamera B]; cams_copied_: its last upload has left it
        hipEvent_t cams_copied_ = nullptr;
        bool remap_both_ = true;    // a prepare with a camera set remaps both images of a pair in one lane (MBAVO_PAIRS_REMAP_BOTH=0: off)
        pairs::CallStats upd_stats_, ass_stats_;
        // the report's scratch, allocated at the first report (not part of the plan): device [blocks B x E | valid B | patch costs
        // B x cap0 | records B], a pinned mirror of the records, the B level-0 problems as the evaluation takes them
        DeviceArray<char> report_;
        PinnedArray<struct mbavo_pairs_report> h_report_;
        std::vector<mbavo_problem> report_probs_;
        pairs::CallStats rep_stats_;
        // the hypotheses' scratch, allocated at the first mbavo_pairs_predict_hypotheses (not part of the plan), sized for 16
        // hypotheses: device [candidate knots_t B x 16 x 3N | knots_R B x 16 x 4N | blocks B x 16 x E | valid B x 16 | records B |
        // options], a pinned mirror [records B | options], the B * M entries as the evaluation takes them
        DeviceArray<char> hyp_;
        PinnedArray<char> h_hyp_;
        std::vector<mbavo_problem> hyp_probs_;
        pairs::CallStats hyp_stats_;
        // the depth stages (not part of the plan; allocated at a stage's first call): one DepthCall each -- the hand-over's two
        // calls share one and count apart -- and the slot layout of their per-keypoint arrays
        pairs::DepthSlots slots_;
        pairs::DepthCall refine_call_{*this}, filter_call_{*this}, search_call_{*this}, smooth_call_{*this}, carry_call_{*this},
            prune_call_{*this}, photo_call_{*this};
        pairs::CallStats csv_stats_, cad_stats_;
        pairs::PhotoCal photocal_;
        pairs::Detector detector_;
        // the filter's state (filter_arrays), handed out once filter_ready_.  kp_serial_: one per pair, bumped where its keypoints
        // are rewritten or pruned; seeded_at_: the serial each (pair, level)'s state was last seeded at (0: never) -- a prune that
        // bumps a pair's serial takes the levels that were current along, as it has moved their state with the keypoints
        DeviceArray<char> filter_state_;
        bool filter_ready_ = false;
        std::vector<unsigned long long> kp_serial_, seeded_at_;
        // pairs_bin_index.h's IndexLayout, then the smoothing's [new depths | new mu] / the hand-over's [staged pixels | rho' | w'].
        // index_serial_, index_s_: the serial and bin edge each index was built at; armed_: per pair its carried set's radius, 0: none
        DeviceArray<char> smooth_index_, carry_set_;
        std::vector<unsigned long long> index_serial_;
        std::vector<int> index_s_, armed_;
        std::vector<mbavo_problem> probs_;
        std::vector<int> start_idx_;  // one per pair, shared by its levels
        pairs::CallStats stats_;
    };
} // namespace mbavo

#endif
