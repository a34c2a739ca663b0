// c_api.cpp -- the extern "C" boundary declared in include/mbavo.h.
// Thin POD wrappers over the C++ ba_tracker API (ba_tracker.h), the fused engine
// (engine.h) and the host control flow (host_math.h, tracker.h, lm_batch.h).
#include "../../include/mbavo.h"
#include "ba_tracker.h"
#include "engine.h"
#include "host_math.h"
#include "lm_batch.h"
#include "pairs_prep.h"
#include "se3_math.h"
#include "tracker.h"
#include "timing.h"
#include "vo_frontend.h"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

using namespace SLAM;

// One helper thread per extra group of mbavo_lm_batch, kept between calls: a job is handed over through a flag the helper
// spins on for a short while after its last job (back-to-back calls: no wake-up latency) before it blocks on a condition variable
// (creating a thread per call cost ~60 us of a 1.2 ms call).
struct GroupWorker
{
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<void()> job;
    std::atomic<int> state{0}; // 0 idle, 1 job posted, 2 job done, 3 exit
    GroupWorker()
    {
        th = std::thread([this]() {
            for (;;)
            {
                int s = state.load(std::memory_order_acquire);
                if (s != 1 && s != 3)
                { // spin ~200 us, then sleep
                    const auto t0 = std::chrono::steady_clock::now();
                    while ((s = state.load(std::memory_order_acquire)) != 1 && s != 3)
                    {
                        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200))
                        {
                            std::unique_lock<std::mutex> lk(m);
                            cv.wait(lk, [&]() { const int v = state.load(std::memory_order_acquire); return v == 1 || v == 3; });
                            s = state.load(std::memory_order_acquire);
                            break;
                        }
                    }
                }
                if (s == 3) return;
                job();
                state.store(2, std::memory_order_release);
            }
        });
    }
    void post(std::function<void()> f)
    {
        job = std::move(f);
        {
            std::lock_guard<std::mutex> lk(m);
            state.store(1, std::memory_order_release);
        }
        cv.notify_one();
    }
    void wait()
    {
        while (state.load(std::memory_order_acquire) != 2) std::this_thread::yield();
        state.store(0, std::memory_order_release);
    }
    ~GroupWorker()
    {
        {
            std::lock_guard<std::mutex> lk(m);
            state.store(3, std::memory_order_release);
        }
        cv.notify_one();
        if (th.joinable()) th.join();
    }
};

struct mbavo_ctx
{
    mbavo::Engine *engine;
    // mbavo_lm_batch on big batches: a second engine on a stream of its own (created at first use), so that two halves of the
    // batch run as independent chains the GPU interleaves
    std::vector<mbavo::Engine *> extra_engines;
    std::vector<hipStream_t> extra_streams;
    std::vector<GroupWorker *> workers;
    hipEvent_t fork = nullptr;
    mbavo::Engine::Options engine_opts; // (new group engines start with the context's options)
    std::vector<mbavo_pairs *> pairs;   // the live pair batches (mbavo_pairs_create): freed with the context
};
struct mbavo_pairs
{
    mbavo_ctx *ctx;
    mbavo::PairBatch impl;
    mbavo_pairs(mbavo_ctx *c) : ctx(c), impl(*c->engine) {}
};
struct mbavo_vo
{
    VO::BlurAwareDirectTracker impl;
    std::vector<std::vector<int>> patterns; // owns the copies the options point to
    mbavo_vo(mbavo::Engine &e, const VO::BlurAwareDirectTrackerOptions &o) : impl(e, o) {}
};
struct mbavo_lm
{
    VO::LevenbergMarquardtStrategy impl;
};
struct mbavo_tr
{
    VO::TrustRegionStepEvaluator impl;
    explicit mbavo_tr(int m) : impl(m) {}
};

static int packed_len(int k)
{
    const int nd = 6 * k + 1;
    return nd * (nd + 1) / 2;
}

extern "C"
{
    const char *mbavo_version(void) { return "mbavo-mi355x 0.2 (gfx950)"; }
    int mbavo_abi_version(void) { return MBAVO_ABI_VERSION; }
    int mbavo_sizeof(int which)
    { // what the library was compiled with, for a binding to check its own mirror of the structs against
        switch (which)
        {
        case 0: return (int)sizeof(mbavo_problem);
        case 1: return (int)sizeof(mbavo_track_opts);
        case 2: return (int)sizeof(mbavo_lm_batch_opts);
        case 3: return (int)sizeof(mbavo_vo_options);
        case 4: return (int)sizeof(mbavo_engine_opts);
        case 5: return (int)sizeof(mbavo_vo_state);
        case 6: return (int)sizeof(mbavo_trace_rec);
        case 7: return (int)sizeof(mbavo_level);
        case 8: return (int)sizeof(mbavo_lm_batch_result);
        case 9: return (int)sizeof(mbavo_vo_info);
        default: return MBAVO_E_ARG;
        }
    }

    int mbavo_packed_len(int k) { return packed_len(k); }

    int mbavo_create(mbavo_ctx **out, int device_id)
    {
        if (!out) return MBAVO_E_ARG;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n)
        {
            fprintf(stderr, "mbavo: no usable HIP device (count=%d, requested %d); there is no CPU fallback\n", n, device_id);
            return MBAVO_E_NODEVICE;
        }
        hipError_t e = hipSetDevice(device_id);
        if (e != hipSuccess) return (int)e;
        mbavo_ctx *c = new (std::nothrow) mbavo_ctx;
        if (!c) return MBAVO_E_ARG;
        c->engine = new mbavo::Engine(device_id);
        *out = c;
        return 0;
    }

    int mbavo_destroy(mbavo_ctx *ctx)
    {
        if (!ctx) return MBAVO_E_ARG;
        for (mbavo_pairs *p : ctx->pairs) delete p;
        delete ctx->engine;
        for (GroupWorker *w : ctx->workers) delete w;
        for (mbavo::Engine *e : ctx->extra_engines) delete e;
        for (hipStream_t s : ctx->extra_streams) (void)hipStreamDestroy(s);
        if (ctx->fork) (void)hipEventDestroy(ctx->fork);
        delete ctx;
        return 0;
    }

    int mbavo_set_stream(mbavo_ctx *ctx, void *s)
    {
        if (!ctx) return MBAVO_E_ARG;
        ctx->engine->set_stream((hipStream_t)s);
        return 0;
    }

    int mbavo_set_engine_opts(mbavo_ctx *ctx, const mbavo_engine_opts *o)
    {
        if (!ctx) return MBAVO_E_ARG;
        mbavo::Engine::Options e;
        if (o)
        {
            e.sample_parallel = o->sample_parallel; e.single_launch = o->single_launch; e.fused_pose = o->fused_pose;
            e.fused_pose_max_samples = o->fused_pose_max_samples; e.persistent = o->persistent; e.prelaunch = o->prelaunch;
            e.tiles_per_cu = o->tiles_per_cu; e.min_tile_pixels = o->min_tile_pixels; e.sp_max_slot_tiles = o->sp_max_slot_tiles;
        }
        ctx->engine->set_options(e);
        for (mbavo::Engine *x : ctx->extra_engines) x->set_options(e);
        ctx->engine_opts = e;
        return 0;
    }

    int mbavo_get_engine_opts(mbavo_ctx *ctx, mbavo_engine_opts *o)
    {
        if (!ctx || !o) return MBAVO_E_ARG;
        const mbavo::Engine::Options &e = ctx->engine->options();
        memset(o, 0, sizeof(*o));
        o->sample_parallel = e.sample_parallel; o->single_launch = e.single_launch; o->fused_pose = e.fused_pose;
        o->fused_pose_max_samples = e.fused_pose_max_samples; o->persistent = e.persistent; o->prelaunch = e.prelaunch;
        o->tiles_per_cu = e.tiles_per_cu; o->min_tile_pixels = e.min_tile_pixels; o->sp_max_slot_tiles = e.sp_max_slot_tiles;
        return 0;
    }

    int mbavo_eval_batch(mbavo_ctx *ctx, int B, const mbavo_problem *probs, int k, int with_hessian,
                         double *d_frame_blocks, double *d_patch_cost, double *d_valid)
    {
        if (!ctx) return MBAVO_E_ARG;
        return ctx->engine->evaluate(B, probs, k, with_hessian != 0, d_frame_blocks, d_patch_cost, d_valid, nullptr);
    }

    int mbavo_eval_batch_merged(mbavo_ctx *ctx, int B, const mbavo_problem *probs, int k, double *d_frame_blocks, double *d_systems,
                                double *d_patch_cost, double *d_valid)
    {
        if (!ctx || !d_systems) return MBAVO_E_ARG;
        ctx->engine->set_merge_target(d_systems);
        const int rc = ctx->engine->evaluate(B, probs, k, true, d_frame_blocks, d_patch_cost, d_valid, nullptr);
        ctx->engine->set_merge_target(nullptr); // (an evaluate() that failed before it took the target must not leave it armed)
        return rc;
    }

    int mbavo_eval(mbavo_ctx *ctx, const mbavo_problem *p, int k, double *h_cost, double *h_H, double *h_g,
                   double *d_patch_blocks)
    {
        if (!ctx || !p || !h_cost || (h_H && !h_g) || !p->h_start_idx) return MBAVO_E_ARG;
        mbavo::Engine &eng = *ctx->engine;
        const int E = packed_len(k);
        const size_t n = (size_t)p->F * E;
        double *h_fb = eng.host_frame_blocks(n); // pinned, device-visible: the finalize kernel writes it directly
        if (!h_fb) return (int)hipErrorOutOfMemory;
        int rc = eng.evaluate(1, p, k, h_H != nullptr, h_fb, nullptr, nullptr, d_patch_blocks);
        if (rc) return rc;
        hipError_t e = hipStreamSynchronize(eng.stream());
        if (e != hipSuccess) return (int)e;
        if (eng.fetch_status() != 0) return MBAVO_E_RANGE;
        mbavo::merge_blocks_host(p->F, k, h_fb, p->h_start_idx, p->N, h_cost, h_H, h_g);
        return 0;
    }

    // ---- the five launchers (the C++ versions abort on HIP errors like a device assert would)
    int mbavo_compute_virtual_camera_poses(int S, int F, const double *d_cap, const double *d_exp, int k, double t0,
                                           double dt, const double *d_kt, const double *d_kR, double *d_poses,
                                           double *d_J_t, double *d_J_R)
    {
        if ((k != 2 && k != 4) || !d_cap || !d_exp || !d_kt || !d_kR || !d_poses || ((d_J_t == nullptr) != (d_J_R == nullptr)))
            return MBAVO_E_ARG;
        VO::compute_virtual_camera_poses(S, F, d_cap, d_exp, k, t0, dt, d_kt, d_kR, d_poses, d_J_t, d_J_R);
        return 0;
    }

    static void fill(Core::VectorX<double, 4> &i4, Core::VectorX<int, 2> &hw, const double intr[4], const int HW[2])
    {
        i4.nDim = 4; hw.nDim = 2;
        for (int i = 0; i < 4; ++i) i4.values[i] = intr[i];
        hw.values[0] = HW[0]; hw.values[1] = HW[1];
    }

    int mbavo_compute_local_patches_xy(int S, int F, const double *d_poses, const void *d_kps, const double *d_z, int K,
                                       const double intr[4], const int HW[2], void *d_out)
    {
        if (!d_poses || !d_kps || !d_z || !intr || !HW || !d_out) return MBAVO_E_ARG;
        Core::VectorX<double, 4> i4; Core::VectorX<int, 2> hw;
        fill(i4, hw, intr, HW);
        VO::compute_local_patches_xy(S, F, d_poses, (const Core::Vector2d *)d_kps, d_z, K, i4, hw, (Core::Vector2d *)d_out);
        return 0;
    }

    int mbavo_compute_pixel_jacobian_residual(const unsigned char *d_I_ref, const float *d_dIxy,
                                              const unsigned char *const *d_I_cur, int S, int F, const double *d_poses,
                                              int k, const double *d_J_t, const double *d_J_R, const void *d_centres,
                                              const double *d_z, int K, const int *d_pattern, int P, const double intr[4],
                                              const int HW[2], double *d_res, double *d_jac)
    {
        if ((k != 2 && k != 4) || !d_I_ref || !d_I_cur || !d_poses || !d_centres || !d_z || !d_pattern || !d_res ||
            (d_jac && (!d_J_t || !d_J_R || !d_dIxy)))
            return MBAVO_E_ARG;
        Core::VectorX<double, 4> i4; Core::VectorX<int, 2> hw;
        fill(i4, hw, intr, HW);
        VO::compute_pixel_jacobian_residual(d_I_ref, d_dIxy, d_I_cur, S, F, d_poses, k, d_J_t, d_J_R,
                                            (const Core::Vector2d *)d_centres, d_z, K, d_pattern, P, i4, hw, nullptr,
                                            d_res, d_jac);
        return 0;
    }

    int mbavo_compute_patch_cost_gradient_hessian(int F, int K, int P, int k, const double *d_res, const double *d_jac,
                                                  double huber_a, double inv, double *d_blocks)
    {
        if ((k != 2 && k != 4) || !d_res || !d_blocks) return MBAVO_E_ARG;
        VO::compute_patch_cost_gradient_hessian(F, K, P, k, d_res, d_jac, huber_a, inv, d_blocks);
        return 0;
    }

    int mbavo_compute_frame_cost_gradient_hessian(int F, int K, int k, const double *d_blocks, int eval_gh,
                                                  const unsigned char *d_flags, double *d_frame_blocks)
    {
        if ((k != 2 && k != 4) || !d_blocks || !d_frame_blocks) return MBAVO_E_ARG;
        VO::compute_frame_cost_gradient_hessian(F, K, k, d_blocks, eval_gh != 0, d_flags, d_frame_blocks);
        return 0;
    }

    int mbavo_merge_hessian_gradient_cost(int F, int k, const double *d_fb, const int *h_start, int N, double *h_cost,
                                          double *h_H, double *h_g)
    {
        if (!d_fb || !h_start || !h_cost || (h_H && !h_g)) return MBAVO_E_ARG;
        VO::merge_hessian_gradient_cost(F, k, d_fb, h_start, N, h_cost, h_H, h_g);
        return 0;
    }

    int mbavo_merge_host(int F, int k, const double *h_fb, const int *h_start, int N, double *h_cost, double *h_H,
                         double *h_g)
    {
        if (!h_fb || !h_start || !h_cost || (h_H && !h_g)) return MBAVO_E_ARG;
        mbavo::merge_blocks_host(F, k, h_fb, h_start, N, h_cost, h_H, h_g);
        return 0;
    }

    int mbavo_solve_normal_equation(const double *A, const double *b, int n, int type, double *x)
    {
        if (!A || !b || !x || n < 1) return MBAVO_E_ARG;
        return mbavo::solve_normal_equation_host(A, b, n, type, x) < 0 ? MBAVO_E_ARG : 0;
    }

    // ---- LM / trust region
    mbavo_lm *mbavo_lm_new(void) { return new mbavo_lm(); }
    void mbavo_lm_delete(mbavo_lm *p) { delete p; }
    void mbavo_lm_reset(mbavo_lm *p) { p->impl.reset(); }
    void mbavo_lm_step_accepted(mbavo_lm *p, double q) { p->impl.step_accepted(q); }
    void mbavo_lm_step_rejected(mbavo_lm *p) { p->impl.step_rejected(); }
    double mbavo_lm_get_radius(mbavo_lm *p) { return p->impl.get_radius(); }
    mbavo_tr *mbavo_tr_new(int m) { return new mbavo_tr(m); }
    void mbavo_tr_delete(mbavo_tr *p) { delete p; }
    void mbavo_tr_reset(mbavo_tr *p, double c) { p->impl.reset(c); }
    double mbavo_tr_step_quality(mbavo_tr *p, double c, double m) { return p->impl.StepQuality(c, m); }
    void mbavo_tr_step_accepted(mbavo_tr *p, double c, double m) { p->impl.StepAccepted(c, m); }

    // ---- spline
    int mbavo_spline_get_pose(int k, double t0, double dt, const double *kt, const double *kR, int N, double t,
                              double t_out[3], double q_out[4], double *J_t, double *J_R)
    {
        if ((k != 2 && k != 4) || !kt || !kR || !t_out || !q_out) return MBAVO_E_ARG;
        Core::SplineSE3 s(t0, dt);
        s.setSplineDegK(k);
        for (int i = 0; i < N; ++i) s.InsertControlKnot(kR + 4 * i, kt + 3 * i);
        return s.GetPose(t, q_out, t_out, J_R, J_t) ? 0 : MBAVO_E_RANGE;
    }

    int mbavo_spline_plus(const double *kt, const double *kR, int N, const double *step, double *cand_t, double *cand_R)
    {
        if (!kt || !kR || !step || !cand_t || !cand_R) return MBAVO_E_ARG;
        Core::SplineSE3 s;
        for (int i = 0; i < N; ++i) s.InsertControlKnot(kR + 4 * i, kt + 3 * i);
        s.Plus_t(step, cand_t);
        s.Plus_R(step + 3 * N, cand_R);
        return 0;
    }

    int mbavo_segment_start_index(double t, double t0, double dt)
    {
        return mbavo::spline_segment_index(t, t0, dt);
    }

    int mbavo_optimize_trajectory(mbavo_ctx *ctx, const mbavo_track_opts *o, const mbavo_level *levels, int F,
                                  const double *h_cap, const double *h_exp, double t0, double dt, double *kt, double *kR,
                                  int N, int *start_idx_out, double *final_cost, mbavo_trace_rec *trace, int cap)
    {
        if (!ctx || !o || !levels || !h_cap || !h_exp || !kt || !kR) return MBAVO_E_ARG;
        return mbavo::optimize_trajectory(*ctx->engine, *o, levels, F, h_cap, h_exp, t0, dt, kt, kR, N, start_idx_out,
                                          final_cost, trace, cap);
    }

    // B pairs of L levels (L = 1: mbavo_lm_batch); the groups split the batch at pair boundaries
    static int lm_batch_groups(mbavo_ctx *ctx, int B, int L, const mbavo_problem *probs, const mbavo_lm_batch_opts *o,
                               mbavo_lm_batch_result *results, mbavo_trace_rec *trace, int trace_cap)
    {
        if (!ctx || !probs || !o || trace_cap < 0) return MBAVO_E_ARG;
        // Big batches as TWO independent groups (round 4): the pairs share nothing, so the halves run
        // the whole loop side by side -- the second on its own engine, stream and host thread -- and the GPU fills one group's
        // solve / decide launches (one latency-bound workgroup per problem, ~35 us of a 512-pair slot) and the ramps and tails of
        // its passes with the other group's kernels.  Measured (rendered 640x480 pairs, us per LM round, one / two / four groups):
        // 512 pairs 159-163 / 144-145 / 145-149 (packed keyframes 143 / 132 / 132-136), 256 pairs 109 / 115, 128 pairs 86 / 102,
        // 64 pairs 74 / 96 -- below ~400 problems a group's passes no longer fill the machine and every phase is latency-bound
        // either way, so smaller batches stay one group.  Two groups of a 512-pair batch keep the single group's tiling (one
        // tile per pair): identical records.  mbavo_lm_batch_opts.groups = n overrides (1 .. 8).
        const int genv = mbavo::read_env_overrides().lm_groups;
        int groups = genv != mbavo::kEnvUnset ? genv : (o->groups > 0 ? o->groups : (B >= 384 ? 2 : 1));
        if (groups > 8) groups = 8;
        if (groups > B) groups = B;
        if (groups < 2)
        {
            try { return mbavo::lm_batch(*ctx->engine, B, L, probs, *o, results, trace, trace_cap); }
            catch (...) { (void)hipStreamSynchronize(ctx->engine->stream()); return MBAVO_E_ARG; }
        }
        // (every group's arguments are checked before the first group starts: an error returns with nothing launched)
        if (mbavo::lm_batch_check(B, L, probs, *o) != 0) return MBAVO_E_ARG;
        const int dev = ctx->engine->device();
        if (hipSetDevice(dev) != hipSuccess) return MBAVO_E_NODEVICE;
        if (!ctx->fork && hipEventCreateWithFlags(&ctx->fork, hipEventDisableTiming) != hipSuccess) return MBAVO_E_NODEVICE;
        while ((int)ctx->extra_engines.size() < groups - 1)
        {
            hipStream_t s = nullptr;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return MBAVO_E_NODEVICE;
            ctx->extra_streams.push_back(s);
            ctx->extra_engines.push_back(new mbavo::Engine(dev));
            ctx->extra_engines.back()->set_stream(s);
            ctx->extra_engines.back()->set_options(ctx->engine_opts);
            ctx->workers.push_back(new GroupWorker());
        }
        // whatever the caller enqueued on the context's stream (knot resets, uploads) comes before the other groups' work too
        if (hipEventRecord(ctx->fork, ctx->engine->stream()) != hipSuccess) return MBAVO_E_NODEVICE;
        // What the whole batch decides is decided ONCE and handed to every group: the largest knot count (array strides,
        // the solve kernel's form -- wide workgroup or one wave -- and its LDS) and the largest sample count.  A group's own list is
        // still tiled for itself, so the grouping of the partial sums -- and with it the last bits of costs and knots -- can differ
        // from the single-group run (as with `retile`); the discrete records do not (tests: mixed N, B just under 2 x CUs).
        const mbavo::LmBatchShared shared = mbavo::LmBatchShared::of(probs, B * L);
        // shared state of the groups lives on the heap and the workers are ALWAYS waited for, also when this thread's own group throws
        // (std::bad_alloc from a vector): no exception crosses the C boundary and no worker writes into a dead frame
        struct Rcs { std::vector<int> v; };
        auto rcs = std::make_shared<Rcs>();
        rcs->v.assign(groups, 0);
        std::vector<int> posted;
        auto first_of = [B, groups](int g) { return (int)((long long)B * g / groups); }; // contiguous, near-equal shares
        const mbavo_lm_batch_opts opts = *o;
        for (int g = 1; g < groups; ++g)
        {
            if (hipStreamWaitEvent(ctx->extra_streams[g - 1], ctx->fork, 0) != hipSuccess) { rcs->v[g] = MBAVO_E_NODEVICE; continue; }
            mbavo::Engine *eng = ctx->extra_engines[g - 1];
            ctx->workers[g - 1]->post([=]() {
                const int b0 = first_of(g), n = first_of(g + 1) - b0;
                int rc;
                try
                {
                    rc = mbavo::lm_batch(*eng, n, L, probs + (size_t)b0 * L, opts, results ? results + b0 : nullptr,
                                         trace ? trace + (size_t)b0 * trace_cap : nullptr, trace_cap, &shared);
                }
                catch (...) { rc = MBAVO_E_ARG; (void)hipStreamSynchronize(eng->stream()); }
                rcs->v[g] = rc;
            });
            posted.push_back(g - 1);
        }
        try
        {
            rcs->v[0] = mbavo::lm_batch(*ctx->engine, first_of(1), L, probs, opts, results, trace, trace_cap, &shared);
        }
        catch (...) { rcs->v[0] = MBAVO_E_ARG; (void)hipStreamSynchronize(ctx->engine->stream()); }
        for (int w : posted) ctx->workers[w]->wait(); // (every call returns synchronised with its streams, failed or not)
        for (int g = 0; g < groups; ++g)
            if (rcs->v[g] != 0) return rcs->v[g];
        return 0;
    }

    int mbavo_lm_batch(mbavo_ctx *ctx, int B, const mbavo_problem *probs, const mbavo_lm_batch_opts *o,
                       mbavo_lm_batch_result *results, mbavo_trace_rec *trace, int trace_cap)
    {
        return lm_batch_groups(ctx, B, 1, probs, o, results, trace, trace_cap);
    }

    int mbavo_lm_batch_levels(mbavo_ctx *ctx, int B, int L, const mbavo_problem *probs, const mbavo_lm_batch_opts *o,
                              mbavo_lm_batch_result *results, mbavo_trace_rec *trace, int trace_cap)
    {
        if (L < 1 || L > 8) return MBAVO_E_ARG;
        return lm_batch_groups(ctx, B, L, probs, o, results, trace, trace_cap);
    }

    // ---- trackFrame front end
    int mbavo_detect_semidense(mbavo_ctx *ctx, const unsigned char *d_img, int H, int W, int level, int H0, int W0, int cell_H,
                               int cell_W, float thr, const float *d_depth_z, double *d_kp_xy, double *d_kp_z, int cap, int *h_count)
    {
        if (!ctx) return MBAVO_E_ARG;
        return mbavo::detect_semidense(*ctx->engine, d_img, H, W, level, H0, W0, cell_H, cell_W, thr, d_depth_z, d_kp_xy, d_kp_z,
                                       cap, h_count);
    }

    int mbavo_depth_to_z(mbavo_ctx *ctx, int depth_format, const void *d_depth, int H, int W, const double intrinsics[4], float depth_unit,
                         float depth_max, float *d_z)
    {
        if (!ctx) return MBAVO_E_ARG;
        return mbavo::depth_to_z(*ctx->engine, depth_format, d_depth, H, W, intrinsics, depth_unit, depth_max, d_z);
    }

    int mbavo_camera_radtan_size(void) { return (int)sizeof(mbavo_camera_radtan); }
    static_assert(sizeof(mbavo_camera_radtan) == 72, "mbavo_camera_radtan: two ints and eight doubles, no padding");

    int mbavo_undistort_map(mbavo_ctx *ctx, const mbavo_camera_radtan *from, const double to_intrinsics[4], int H, int W, float *d_map_xy)
    {
        if (!ctx) return MBAVO_E_ARG;
        return mbavo::undistort_map(*ctx->engine, from, to_intrinsics, H, W, d_map_xy);
    }

    int mbavo_undistort_u8(mbavo_ctx *ctx, const unsigned char *d_src, int Hs, int Ws, const float *d_map_xy, int H, int W, unsigned char *d_dst)
    {
        if (!ctx) return MBAVO_E_ARG;
        return mbavo::undistort_u8(*ctx->engine, d_src, Hs, Ws, d_map_xy, H, W, d_dst);
    }

    int mbavo_camera_unified_size(void) { return (int)sizeof(mbavo_camera_unified); }
    static_assert(sizeof(mbavo_camera_unified) == 80, "mbavo_camera_unified: two ints and nine doubles, no padding");

    int mbavo_undistort_map_unified(mbavo_ctx *ctx, const mbavo_camera_unified *from, const double to_intrinsics[4], int H, int W, float *d_map_xy)
    {
        if (!ctx) return MBAVO_E_ARG;
        return mbavo::undistort_map_unified(*ctx->engine, from, to_intrinsics, H, W, d_map_xy);
    }

    int mbavo_undistort_u8_batch(mbavo_ctx *ctx, const unsigned char *d_src, int n, int Hs, int Ws, const float *d_map_xy, int H, int W,
                                 unsigned char *d_dst)
    {
        if (!ctx) return MBAVO_E_ARG;
        return mbavo::undistort_u8_batch(*ctx->engine, d_src, n, Hs, Ws, d_map_xy, H, W, d_dst);
    }

    int mbavo_pyramid_levels_u8(mbavo_ctx *ctx, unsigned char *const *h_level_ptrs, int H0, int W0, int num_levels)
    {
        if (!ctx || !h_level_ptrs || num_levels < 1 || num_levels > 8) return MBAVO_E_ARG;
        for (int l = 0; l < num_levels; ++l)
            if (!h_level_ptrs[l]) return MBAVO_E_ARG;
        return mbavo::pyramid_enqueue(*ctx->engine, h_level_ptrs, H0, W0, num_levels);
    }

    // ---- the input side of a batch of pairs (pairs_prep.hip)
    int mbavo_pairs_opts_size(void) { return (int)sizeof(mbavo_pairs_opts); }
    static_assert(sizeof(mbavo_pairs_opts) == 272, "mbavo_pairs_opts: the depth fields, `undistort` and `num_cameras` came out of `reserved`, the size stays");
    static_assert(offsetof(mbavo_pairs_opts, mask) == 268, "mbavo_pairs_opts.mask is the last word, the one `reserved2` names");

    int mbavo_pairs_plan(const mbavo_pairs_opts *o, long long *h_device_bytes, int h_cells_per_level[8])
    {
        if (!o || !h_device_bytes || !h_cells_per_level) return MBAVO_E_ARG;
        mbavo::PairsPlan plan;
        const int rc = mbavo::pairs_plan(o, plan);
        if (rc != 0) return rc;
        *h_device_bytes = plan.total;
        for (int l = 0; l < 8; ++l) h_cells_per_level[l] = l < plan.L ? plan.cap[l] : 0;
        return 0;
    }

    int mbavo_pairs_create(mbavo_ctx *ctx, const mbavo_pairs_opts *o, mbavo_pairs **out)
    {
        if (!ctx || !o || !out) return MBAVO_E_ARG;
        mbavo_pairs *p = new (std::nothrow) mbavo_pairs(ctx);
        if (!p) return (int)hipErrorOutOfMemory;
        int rc;
        try { rc = p->impl.create(o); } // (validates first: bad options allocate nothing and launch nothing)
        catch (const std::bad_alloc &) { rc = (int)hipErrorOutOfMemory; }
        catch (...) { rc = MBAVO_E_ARG; }
        if (rc != 0) { delete p; return rc; }
        ctx->pairs.push_back(p);
        *out = p;
        return 0;
    }

    int mbavo_pairs_destroy(mbavo_pairs *p)
    {
        if (!p) return MBAVO_E_ARG;
        std::vector<mbavo_pairs *> &v = p->ctx->pairs;
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i] == p) { v.erase(v.begin() + i); break; }
        delete p;
        return 0;
    }

    int mbavo_pairs_prepare(mbavo_pairs *p, const unsigned char *d_sharp, const float *d_depth_z, const unsigned char *d_blur, int *h_counts)
    {
        return p ? p->impl.prepare(d_sharp, d_depth_z, d_blur, h_counts) : MBAVO_E_ARG;
    }

    int mbavo_pairs_prepare_points(mbavo_pairs *p, const unsigned char *d_sharp, const unsigned char *d_blur, const int *h_offsets, const double *d_xy,
                                   const double *d_z, int *h_counts)
    {
        return p ? p->impl.prepare_points(d_sharp, d_blur, h_offsets, d_xy, d_z, h_counts) : MBAVO_E_ARG;
    }

    int mbavo_pairs_set_camera(mbavo_pairs *p, const mbavo_camera_radtan *from) { return p ? p->impl.set_camera(from) : MBAVO_E_ARG; }
    int mbavo_pairs_set_camera_unified(mbavo_pairs *p, const mbavo_camera_unified *from) { return p ? p->impl.set_camera(from) : MBAVO_E_ARG; }

    int mbavo_pairs_camera_size(void) { return (int)sizeof(mbavo_pairs_camera); }
    static_assert(sizeof(mbavo_pairs_camera) == 120, "mbavo_pairs_camera: four ints and thirteen doubles, no padding");
    int mbavo_pairs_set_cameras(mbavo_pairs *p, int G, const mbavo_pairs_camera *h_cams, const int *h_camera_of_pair)
    {
        if (!p) return MBAVO_E_ARG;
        try { return p->impl.set_cameras(G, h_cams, h_camera_of_pair); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }
    int mbavo_undistort_map_batch(mbavo_ctx *ctx, int n, const mbavo_pairs_camera *h_cams, int H, int W, float *d_maps)
    {
        if (!ctx) return MBAVO_E_ARG;
        try { return mbavo::undistort_map_batch(*ctx->engine, n, h_cams, H, W, d_maps); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    int mbavo_undistort_points_batch(mbavo_ctx *ctx, int n_cams, const mbavo_pairs_camera *h_cams, const int *h_offsets, const double *d_uv,
                                     double *d_xy, unsigned char *d_ok_or_null)
    {
        if (!ctx) return MBAVO_E_ARG;
        try { return mbavo::undistort_points_batch(*ctx->engine, n_cams, h_cams, h_offsets, d_uv, d_xy, d_ok_or_null); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }
    int mbavo_pairs_set_points_geometry(mbavo_pairs *p, int geometry) { return p ? p->impl.set_points_geometry(geometry) : MBAVO_E_ARG; }

    int mbavo_undistort_clearance_batch(mbavo_ctx *ctx, int n, const float *d_maps, int H, int W, int Hs, int Ws, int L, int radius,
                                        unsigned char *d_clear)
    {
        if (!ctx) return MBAVO_E_ARG;
        return mbavo::undistort_clearance_batch(*ctx->engine, n, d_maps, H, W, Hs, Ws, L, radius, d_clear);
    }
    int mbavo_mask_clearance_batch(mbavo_ctx *ctx, int n, const float *d_maps, const unsigned char *d_masks, int H, int W, int Hs, int Ws, int L,
                                   int radius, unsigned char *d_clear)
    {
        if (!ctx) return MBAVO_E_ARG;
        return mbavo::mask_clearance_batch(*ctx->engine, n, d_maps, d_masks, H, W, Hs, Ws, L, radius, d_clear);
    }
    int mbavo_undistort_mask_batch(mbavo_ctx *ctx, int n, const unsigned char *d_raw_masks, int Hs, int Ws, const float *d_maps, int H, int W,
                                   unsigned char *d_masks_out)
    {
        if (!ctx) return MBAVO_E_ARG;
        return mbavo::undistort_mask_batch(*ctx->engine, n, d_raw_masks, Hs, Ws, d_maps, H, W, d_masks_out);
    }
    int mbavo_pairs_set_masks(mbavo_pairs *p, int geometry, int n, const unsigned char *d_masks)
    {
        return p ? p->impl.set_masks(geometry, n, d_masks) : MBAVO_E_ARG;
    }
    long long mbavo_undistort_clearance_bytes(int H, int W, int L)
    {
        mbavo::ClearLevels lv;
        const int rc = mbavo::clear_levels(H, W, L, 1, lv);
        return rc != 0 ? (long long)rc : lv.stride;
    }

    int mbavo_pairs_set_motion(mbavo_pairs *p, const double *h_cap, const double *h_exp, const double *h_t0, double dt, const double *h_kt,
                               const double *h_kR)
    {
        return p ? p->impl.set_motion(h_cap, h_exp, h_t0, dt, h_kt, h_kR) : MBAVO_E_ARG;
    }

    int mbavo_pairs_get_knots(mbavo_pairs *p, double *h_kt, double *h_kR) { return p ? p->impl.get_knots(h_kt, h_kR) : MBAVO_E_ARG; }

    int mbavo_pairs_problems(mbavo_pairs *p, const mbavo_problem **h_out, int *h_count)
    {
        if (!p || !h_out) return MBAVO_E_ARG;
        *h_out = p->impl.problems();
        if (h_count) *h_count = p->impl.count();
        return 0;
    }

    int mbavo_pairs_last_stats(mbavo_pairs *p, long long out[4])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.last_stats(out);
        return 0;
    }

    int mbavo_pairs_assessment_size(void) { return (int)sizeof(mbavo_pairs_assessment); }

    int mbavo_pairs_assess(mbavo_pairs *p, double flow_mag0, double flow_mag1, double max_blur_kernel_mag, mbavo_pairs_assessment *h_out)
    {
        return p ? p->impl.assess(flow_mag0, flow_mag1, max_blur_kernel_mag, h_out) : MBAVO_E_ARG;
    }

    int mbavo_pairs_assess_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.assess_stats(out);
        return 0;
    }

    int mbavo_pairs_update(mbavo_pairs *p, const unsigned char *d_blur, int n_key, const int *h_key_pairs, const unsigned char *d_sharp,
                           const float *d_depth_z, int *h_counts)
    {
        return p ? p->impl.update(d_blur, n_key, h_key_pairs, d_sharp, d_depth_z, h_counts) : MBAVO_E_ARG;
    }

    int mbavo_pairs_update_points(mbavo_pairs *p, const unsigned char *d_blur, int n_key, const int *h_key_pairs, const unsigned char *d_sharp,
                                  const int *h_offsets, const double *d_xy, const double *d_z, int *h_counts)
    {
        return p ? p->impl.update_points(d_blur, n_key, h_key_pairs, d_sharp, h_offsets, d_xy, d_z, h_counts) : MBAVO_E_ARG;
    }

    int mbavo_pairs_update_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.update_stats(out);
        return 0;
    }

    // ---- tracker state of a batch of pairs on the device (pairs_track.hip)
    int mbavo_pairs_frame_size(void) { return (int)sizeof(mbavo_pairs_frame); }
    static_assert(sizeof(mbavo_pairs_frame) == 144, "mbavo_pairs_frame: an assessment and a pose, no padding");

    int mbavo_pairs_set_states(mbavo_pairs *p, const mbavo_vo_state *h_states) { return p ? p->impl.set_states(h_states) : MBAVO_E_ARG; }
    int mbavo_pairs_get_states(mbavo_pairs *p, mbavo_vo_state *h_states) { return p ? p->impl.get_states(h_states) : MBAVO_E_ARG; }
    int mbavo_pairs_predict(mbavo_pairs *p, const double *h_cap, const double *h_exp) { return p ? p->impl.predict(h_cap, h_exp) : MBAVO_E_ARG; }
    int mbavo_pairs_commit(mbavo_pairs *p, double flow_mag0, double flow_mag1, double max_blur_kernel_mag, mbavo_pairs_frame *h_out)
    {
        return p ? p->impl.commit(flow_mag0, flow_mag1, max_blur_kernel_mag, h_out) : MBAVO_E_ARG;
    }
    int mbavo_pairs_track_stats(mbavo_pairs *p, long long out[6])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.track_stats(out);
        return 0;
    }

    int mbavo_pairs_track_frame(mbavo_pairs *p, const unsigned char *d_blur, int n_key, const int *h_key_pairs, const unsigned char *d_sharp,
                                const float *d_depth_z, const double *h_cap, const double *h_exp, const mbavo_lm_batch_opts *o,
                                mbavo_lm_batch_result *results, mbavo_trace_rec *trace, int trace_cap, double flow_mag0, double flow_mag1,
                                double max_blur_kernel_mag, mbavo_pairs_frame *h_out, int *h_counts)
    { // the four calls of a frame, in order; the first error ends it
        if (!p || !h_cap || !h_exp || !o || !h_out) return MBAVO_E_ARG;
        int rc = p->impl.update(d_blur, n_key, h_key_pairs, d_sharp, d_depth_z, h_counts);
        if (rc != 0) return rc;
        if ((rc = p->impl.predict(h_cap, h_exp)) != 0) return rc;
        if ((rc = mbavo_lm_batch_levels(p->ctx, p->impl.pairs(), p->impl.levels(), p->impl.problems(), o, results, trace, trace_cap)) != 0) return rc;
        return p->impl.commit(flow_mag0, flow_mag1, max_blur_kernel_mag, h_out);
    }

    int mbavo_pairs_track_frame_points(mbavo_pairs *p, const unsigned char *d_blur, int n_key, const int *h_key_pairs, const unsigned char *d_sharp,
                                       const int *h_offsets, const double *d_xy, const double *d_z, const double *h_cap, const double *h_exp,
                                       const mbavo_lm_batch_opts *o, mbavo_lm_batch_result *results, mbavo_trace_rec *trace, int trace_cap,
                                       double flow_mag0, double flow_mag1, double max_blur_kernel_mag, mbavo_pairs_frame *h_out, int *h_counts)
    { // the same four calls with the caller's points for the new keyframes
        if (!p || !h_cap || !h_exp || !o || !h_out) return MBAVO_E_ARG;
        int rc = p->impl.update_points(d_blur, n_key, h_key_pairs, d_sharp, h_offsets, d_xy, d_z, h_counts);
        if (rc != 0) return rc;
        if ((rc = p->impl.predict(h_cap, h_exp)) != 0) return rc;
        if ((rc = mbavo_lm_batch_levels(p->ctx, p->impl.pairs(), p->impl.levels(), p->impl.problems(), o, results, trace, trace_cap)) != 0) return rc;
        return p->impl.commit(flow_mag0, flow_mag1, max_blur_kernel_mag, h_out);
    }

    // ---- pose information, covariance and keypoint flags of a batch of pairs (pairs_report.hip)
    int mbavo_pairs_report_size(void) { return (int)sizeof(struct mbavo_pairs_report); }
    static_assert(sizeof(struct mbavo_pairs_report) == 672, "mbavo_pairs_report: four ints and 82 doubles, no padding");

    int mbavo_pairs_report(mbavo_pairs *p, double max_chi_square_error, struct mbavo_pairs_report *h_out, double *d_patch_cost,
                           unsigned char *d_flags)
    {
        if (!p) return MBAVO_E_ARG;
        try { return p->impl.report(max_chi_square_error, h_out, d_patch_cost, d_flags); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    int mbavo_pairs_report_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.report_stats(out);
        return 0;
    }

    // ---- every pair's start picked among M motion hypotheses (pairs_hyp.hip)
    int mbavo_pairs_hyp_opts_size(void) { return (int)sizeof(mbavo_pairs_hyp_opts); }
    int mbavo_pairs_hyp_size(void) { return (int)sizeof(mbavo_pairs_hyp); }
    static_assert(sizeof(mbavo_pairs_hyp_opts) == 936, "mbavo_pairs_hyp_opts: two ints, 114 doubles, four ints, no padding");
    static_assert(sizeof(mbavo_pairs_hyp) == 272, "mbavo_pairs_hyp: four ints and 32 doubles, no padding");

    int mbavo_pairs_predict_hypotheses(mbavo_pairs *p, const double *h_cap, const double *h_exp, const mbavo_pairs_hyp_opts *opts,
                                       mbavo_pairs_hyp *h_out)
    {
        if (!p) return MBAVO_E_ARG;
        try { return p->impl.predict_hypotheses(h_cap, h_exp, opts, h_out); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    int mbavo_pairs_hyp_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.hyp_stats(out);
        return 0;
    }

    // ---- every keypoint's depth gradient, curvature and damped inverse-depth step (pairs_refine.hip)
    int mbavo_pairs_refine_opts_size(void) { return (int)sizeof(mbavo_pairs_refine_opts); }
    int mbavo_pairs_refine_size(void) { return (int)sizeof(struct mbavo_pairs_refine); }
    static_assert(sizeof(mbavo_pairs_refine_opts) == 56, "mbavo_pairs_refine_opts: two ints, four doubles, four ints, no padding");
    static_assert(sizeof(struct mbavo_pairs_refine) == 32, "mbavo_pairs_refine: four ints and two doubles, no padding");

    int mbavo_pairs_refine_depths(mbavo_pairs *p, const mbavo_pairs_refine_opts *opts, struct mbavo_pairs_refine *h_out, double *d_g, double *d_h,
                                  double *d_cost, int *d_valid)
    {
        if (!p) return MBAVO_E_ARG;
        try { return p->impl.refine_depths(opts, h_out, d_g, d_h, d_cost, d_valid); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    int mbavo_pairs_refine_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.refine_stats(out);
        return 0;
    }

    // ---- the recursive inverse-depth filter of every keypoint over the frames of its keyframe (pairs_filter.hip)
    int mbavo_pairs_filter_opts_size(void) { return (int)sizeof(mbavo_pairs_filter_opts); }
    int mbavo_pairs_filter_size(void) { return (int)sizeof(struct mbavo_pairs_filter); }
    static_assert(sizeof(mbavo_pairs_filter_opts) == 96, "mbavo_pairs_filter_opts: two ints, seven doubles, eight ints, no padding");
    static_assert(sizeof(struct mbavo_pairs_filter) == 48, "mbavo_pairs_filter: six ints and three doubles, no padding");

    int mbavo_pairs_filter_depths(mbavo_pairs *p, const mbavo_pairs_filter_opts *opts, struct mbavo_pairs_filter *h_out)
    {
        if (!p) return MBAVO_E_ARG;
        try { return p->impl.filter_depths(opts, h_out); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    int mbavo_pairs_filter_state(mbavo_pairs *p, double **d_mu, double **d_info, int **d_n_obs, int **d_n_rej, long long *h_pair_stride,
                                 long long h_level_offset[8])
    {
        return p ? p->impl.filter_state(d_mu, d_info, d_n_obs, d_n_rej, h_pair_stride, h_level_offset) : MBAVO_E_ARG;
    }

    int mbavo_pairs_filter_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.filter_stats(out);
        return 0;
    }

    // ---- every keypoint's depth searched among ND inverse-depth candidates (pairs_search.hip)
    int mbavo_pairs_search_opts_size(void) { return (int)sizeof(mbavo_pairs_search_opts); }
    int mbavo_pairs_search_size(void) { return (int)sizeof(struct mbavo_pairs_search); }
    static_assert(sizeof(mbavo_pairs_search_opts) == 80, "mbavo_pairs_search_opts: four ints, six doubles, four ints, no padding");
    static_assert(sizeof(struct mbavo_pairs_search) == 32, "mbavo_pairs_search: four ints and two doubles, no padding");

    int mbavo_pairs_search_depths(mbavo_pairs *p, const mbavo_pairs_search_opts *opts, struct mbavo_pairs_search *h_out, double *d_rho,
                                  double *d_cost_best, double *d_cost_second, double *d_curv, int *d_best, int *d_num_full, double *d_volume)
    {
        if (!p) return MBAVO_E_ARG;
        try { return p->impl.search_depths(opts, h_out, d_rho, d_cost_best, d_cost_second, d_curv, d_best, d_num_full, d_volume); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    int mbavo_pairs_search_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.search_stats(out);
        return 0;
    }

    // ---- every pair's brightness gain and offset, fitted and removed (pairs_photo.hip)
    int mbavo_pairs_photo_opts_size(void) { return (int)sizeof(mbavo_pairs_photo_opts); }
    int mbavo_pairs_photo_size(void) { return (int)sizeof(struct mbavo_pairs_photo); }
    static_assert(sizeof(mbavo_pairs_photo_opts) == 64, "mbavo_pairs_photo_opts: four ints, four doubles, four ints, no padding");
    static_assert(sizeof(struct mbavo_pairs_photo) == 48, "mbavo_pairs_photo: four ints and four doubles, no padding");

    int mbavo_pairs_match_brightness(mbavo_pairs *p, const mbavo_pairs_photo_opts *opts, struct mbavo_pairs_photo *h_out)
    {
        if (!p) return MBAVO_E_ARG;
        try { return p->impl.match_brightness(opts, h_out); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    int mbavo_pairs_photo_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.photo_stats(out);
        return 0;
    }

    // ---- the sensor's photometric calibration at intake (pairs_photocal.hip)
    int mbavo_pairs_photocal_opts_size(void) { return (int)sizeof(mbavo_pairs_photocal_opts); }
    static_assert(sizeof(mbavo_pairs_photocal_opts) == 32, "mbavo_pairs_photocal_opts: a double, a float and five ints, no padding");

    int mbavo_photometric_table(const double *h_G, double scale, float *h_lut) { return mbavo::photometric_table(h_G, scale, h_lut); }

    int mbavo_pairs_set_photometric(mbavo_pairs *p, int n, const double *h_G, const float *d_vignette, const mbavo_pairs_photocal_opts *opts)
    {
        if (!p) return MBAVO_E_ARG;
        try { return p->impl.set_photometric(n, h_G, d_vignette, opts); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    int mbavo_pairs_clear_photometric(mbavo_pairs *p) { return p ? p->impl.clear_photometric() : MBAVO_E_ARG; }

    int mbavo_pairs_photocal_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.photocal_stats(out);
        return 0;
    }

    // ---- keypoints by corner strength (pairs_score.hip, which also defines mbavo_corner_score_u8)
    int mbavo_pairs_detector_opts_size(void) { return (int)sizeof(mbavo_pairs_detector_opts); }
    static_assert(sizeof(mbavo_pairs_detector_opts) == 32, "mbavo_pairs_detector_opts: two ints, a float and five ints, no padding");

    int mbavo_pairs_set_detector(mbavo_pairs *p, const mbavo_pairs_detector_opts *opts) { return p ? p->impl.set_detector(opts) : MBAVO_E_ARG; }

    int mbavo_pairs_detector_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.detector_stats(out);
        return 0;
    }

    int mbavo_photometric_u8_batch(mbavo_ctx *ctx, int n_img, const unsigned char *d_src, int H, int W, int n_cal, const float *h_luts,
                                   const float *d_inv, const int *h_cal_of_image, unsigned char *d_dst)
    {
        if (!ctx) return MBAVO_E_ARG;
        try { return mbavo::photometric_u8_batch(*ctx->engine, n_img, d_src, H, W, n_cal, h_luts, d_inv, h_cal_of_image, d_dst); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    // ---- every keypoint's depth smoothed over its image neighbours (pairs_smooth.hip)
    int mbavo_pairs_smooth_opts_size(void) { return (int)sizeof(mbavo_pairs_smooth_opts); }
    int mbavo_pairs_smooth_size(void) { return (int)sizeof(struct mbavo_pairs_smooth); }
    static_assert(sizeof(mbavo_pairs_smooth_opts) == 80, "mbavo_pairs_smooth_opts: eight ints, four doubles, four ints, no padding");
    static_assert(sizeof(struct mbavo_pairs_smooth) == 40, "mbavo_pairs_smooth: six ints, a long long and a double, no padding");

    int mbavo_pairs_smooth_depths(mbavo_pairs *p, const mbavo_pairs_smooth_opts *opts, struct mbavo_pairs_smooth *h_out, const double *d_weight,
                                  double *d_rho, unsigned char *d_flags, int *d_support)
    {
        if (!p) return MBAVO_E_ARG;
        try { return p->impl.smooth_depths(opts, h_out, d_weight, d_rho, d_flags, d_support); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    int mbavo_pairs_smooth_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.smooth_stats(out);
        return 0;
    }

    // ---- keypoint depths and filter state handed to the pair's next keyframe (pairs_carry.hip)
    int mbavo_pairs_carry_save_opts_size(void) { return (int)sizeof(mbavo_pairs_carry_save_opts); }
    int mbavo_pairs_carry_save_size(void) { return (int)sizeof(struct mbavo_pairs_carry_save); }
    int mbavo_pairs_carry_adopt_opts_size(void) { return (int)sizeof(mbavo_pairs_carry_adopt_opts); }
    int mbavo_pairs_carry_adopt_size(void) { return (int)sizeof(struct mbavo_pairs_carry_adopt); }
    static_assert(sizeof(mbavo_pairs_carry_save_opts) == 48, "mbavo_pairs_carry_save_opts: two ints, three doubles, four ints, no padding");
    static_assert(sizeof(struct mbavo_pairs_carry_save) == 24, "mbavo_pairs_carry_save: four ints and a double, no padding");
    static_assert(sizeof(mbavo_pairs_carry_adopt_opts) == 72, "mbavo_pairs_carry_adopt_opts: four ints, five doubles, four ints, no padding");
    static_assert(sizeof(struct mbavo_pairs_carry_adopt) == 32, "mbavo_pairs_carry_adopt: four ints and two doubles, no padding");

    int mbavo_pairs_carry_save(mbavo_pairs *p, int n, const int *h_pairs, const double *h_T, const mbavo_pairs_carry_save_opts *opts,
                               struct mbavo_pairs_carry_save *h_out)
    {
        if (!p) return MBAVO_E_ARG;
        try { return p->impl.carry_save(n, h_pairs, h_T, opts, h_out); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    int mbavo_pairs_carry_adopt(mbavo_pairs *p, int n, const int *h_pairs, const mbavo_pairs_carry_adopt_opts *opts,
                                struct mbavo_pairs_carry_adopt *h_out, double *d_rho, double *d_info, int *d_count, unsigned char *d_flags)
    {
        if (!p) return MBAVO_E_ARG;
        try { return p->impl.carry_adopt(n, h_pairs, opts, h_out, d_rho, d_info, d_count, d_flags); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    int mbavo_pairs_carry_save_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.carry_save_stats(out);
        return 0;
    }

    int mbavo_pairs_carry_adopt_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.carry_adopt_stats(out);
        return 0;
    }

    // ---- flagged keypoints pruned on the device, their state moved along (pairs_prune.hip)
    int mbavo_pairs_prune_opts_size(void) { return (int)sizeof(mbavo_pairs_prune_opts); }
    int mbavo_pairs_prune_size(void) { return (int)sizeof(struct mbavo_pairs_prune); }
    static_assert(sizeof(mbavo_pairs_prune_opts) == 72, "mbavo_pairs_prune_opts: four ints, a double, two ints, two doubles, six ints, no padding");
    static_assert(sizeof(struct mbavo_pairs_prune) == 32, "mbavo_pairs_prune: eight ints, no padding");

    int mbavo_pairs_prune_keypoints(mbavo_pairs *p, int n, const int *h_pairs, const mbavo_pairs_prune_opts *opts, const unsigned char *d_flags,
                                    struct mbavo_pairs_prune *h_out, unsigned char *d_keep)
    {
        if (!p) return MBAVO_E_ARG;
        try { return p->impl.prune_keypoints(n, h_pairs, opts, d_flags, h_out, d_keep); }
        catch (const std::bad_alloc &) { return (int)hipErrorOutOfMemory; }
    }

    int mbavo_pairs_prune_stats(mbavo_pairs *p, long long out[3])
    {
        if (!p || !out) return MBAVO_E_ARG;
        p->impl.prune_stats(out);
        return 0;
    }

    int mbavo_se3_exp(const double a[6], double pose[7])
    {
        if (!a || !pose) return MBAVO_E_ARG;
        memcpy(pose, Core::Transformation::exp(a).getData(), sizeof(double) * 7);
        return 0;
    }
    int mbavo_se3_log(const double pose[7], double out[6])
    {
        if (!pose || !out) return MBAVO_E_ARG;
        Core::Transformation::log(Core::Transformation(pose + 3, pose), out);
        return 0;
    }
    int mbavo_transform_mul(const double A[7], const double B[7], double out[7])
    {
        if (!A || !B || !out) return MBAVO_E_ARG;
        const Core::Transformation r = Core::Transformation(A + 3, A) * Core::Transformation(B + 3, B);
        memcpy(out, r.getData(), sizeof(double) * 7);
        return 0;
    }
    int mbavo_transform_inverse(const double A[7], double out[7])
    {
        if (!A || !out) return MBAVO_E_ARG;
        memcpy(out, Core::Transformation(A + 3, A).inverse().getData(), sizeof(double) * 7);
        return 0;
    }
    int mbavo_spline_transform_to(int k, double t0, double dt, double *kt, double *kR, int N, double t, const double q[4],
                                  const double p[3])
    {
        if ((k != 2 && k != 4) || !kt || !kR || !q || !p || N < k) return MBAVO_E_ARG;
        Core::SplineSE3 s(t0, dt);
        s.setSplineDegK(k);
        for (int i = 0; i < N; ++i) s.InsertControlKnot(kR + 4 * i, kt + 3 * i);
        if (!s.TransformTo(t, q, p)) return MBAVO_E_RANGE;
        memcpy(kt, s.get_knot_data_t(), sizeof(double) * 3 * N);
        memcpy(kR, s.get_knot_data_R(), sizeof(double) * 4 * N);
        return 0;
    }

    int mbavo_spline_transform_by_right(double *kt, double *kR, int N, const double q[4], const double p[3])
    {
        if (!kt || !kR || !q || !p || N < 0) return MBAVO_E_ARG;
        Core::SplineSE3 s;
        for (int i = 0; i < N; ++i) s.InsertControlKnot(kR + 4 * i, kt + 3 * i);
        s.TransformByRight(q, p);
        memcpy(kt, s.get_knot_data_t(), sizeof(double) * 3 * N);
        memcpy(kR, s.get_knot_data_R(), sizeof(double) * 4 * N);
        return 0;
    }

    int mbavo_vo_create(mbavo_ctx *ctx, const mbavo_vo_options *o, mbavo_vo **out)
    {
        if (!ctx || !o || !out || o->num_pyramid_levels < 1 || o->num_pyramid_levels > 8) return MBAVO_E_ARG;
        VO::BlurAwareDirectTrackerOptions v;
        for (int i = 0; i < 4; ++i) v.intrinsics[i] = o->intrinsics[i];
        v.im_size_HW[0] = o->H; v.im_size_HW[1] = o->W;
        v.num_pyramid_levels = o->num_pyramid_levels;
        std::vector<std::vector<int>> pats(8);
        for (int l = 0; l < 8; ++l)
        {
            v.num_virtual_poses_per_frame[l] = o->num_virtual_poses_per_frame[l];
            v.patch_size[l] = o->patch_size[l];
            v.local_patch_pattern_xy[l] = nullptr;
            if (l < o->num_pyramid_levels)
            {
                if (!o->local_patch_pattern_xy[l] || o->patch_size[l] < 1) return MBAVO_E_ARG;
                pats[l].assign(o->local_patch_pattern_xy[l], o->local_patch_pattern_xy[l] + 2 * o->patch_size[l]);
                v.local_patch_pattern_xy[l] = pats[l].data();
            }
        }
        v.huber_k = o->huber_k;
        v.max_consecutive_nonmonotonic_steps = o->max_consecutive_nonmonotonic_steps;
        v.max_num_iterations = o->max_num_iterations;
        v.min_step_quality = o->min_step_quality; v.min_abs_cost_decrease = o->min_abs_cost_decrease;
        v.solver_type = o->solver_type; v.spline_deg_k = o->spline_deg_k;
        v.dt_frame = o->dt_frame; v.dt_ctrl_knot = o->dt_ctrl_knot; v.max_chi_square_error = o->max_chi_square_error;
        v.keyframe_max_flow_mag0 = o->keyframe_max_flow_mag0; v.keyframe_max_flow_mag1 = o->keyframe_max_flow_mag1;
        v.keyframe_max_flow_mag2 = o->keyframe_max_flow_mag2; v.keyframe_max_blur_kernel_mag = o->keyframe_max_blur_kernel_mag;
        v.score_threshold = o->score_threshold;
        v.grid_selection_cell_H = o->grid_selection_cell_H; v.grid_selection_cell_W = o->grid_selection_cell_W;
        v.fast_solve_ratio = o->fast_solve_ratio; v.speculate = o->speculate; v.persist_levels = o->persist_levels;
        v.keyframe_levels_at_once = o->keyframe_levels_at_once; v.speculate_keyframe = o->speculate_keyframe; v.ride_along = o->ride_along; v.resum = o->resum;
        if (v.spline_deg_k != 2 && v.spline_deg_k != 4) return MBAVO_E_ARG;
        mbavo_vo *h = new (std::nothrow) mbavo_vo(*ctx->engine, v);
        if (!h) return MBAVO_E_ARG;
        const int st = h->impl.status();
        if (st != 0) { delete h; return st; }
        h->patterns.swap(pats);
        *out = h;
        return 0;
    }

    int mbavo_vo_destroy(mbavo_vo *vo)
    {
        delete vo;
        return 0;
    }

    int mbavo_vo_set_spline(mbavo_vo *vo, double t0, double dt, int N, const double *kt, const double *kR)
    {
        if (!vo || N < 0 || N > 16 || (N > 0 && (!kt || !kR))) return MBAVO_E_ARG;
        Core::SplineSE3 *s = vo->impl.getSplineTrajectory();
        s->Clear();
        s->setStartTime(t0); s->setSamplingFreq(dt); s->setSplineDegK(vo->impl.getOptions().spline_deg_k);
        for (int i = 0; i < N; ++i) s->InsertControlKnot(kR + 4 * i, kt + 3 * i);
        return 0;
    }

    int mbavo_vo_get_spline(mbavo_vo *vo, double *t0, double *dt, int *N, double *kt, double *kR)
    {
        if (!vo) return MBAVO_E_ARG;
        Core::SplineSE3 *s = vo->impl.getSplineTrajectory();
        const int n = (int)s->get_num_knots();
        if (t0) *t0 = s->getStartTime();
        if (dt) *dt = s->getSamplingFreq();
        if (N) *N = n;
        if (kt && n) memcpy(kt, s->get_knot_data_t(), sizeof(double) * 3 * n);
        if (kR && n) memcpy(kR, s->get_knot_data_R(), sizeof(double) * 4 * n);
        return 0;
    }

    int mbavo_vo_last_trace(mbavo_vo *vo, mbavo_trace_rec *trace, int trace_cap)
    {
        if (!vo || trace_cap < 0 || (trace_cap > 0 && !trace)) return MBAVO_E_ARG;
        return vo->impl.lastTrace(trace, trace_cap);
    }

    static_assert(sizeof(mbavo_vo_state) == sizeof(VO::TrackerState), "mbavo_vo_state mirrors VO::TrackerState");

    int mbavo_vo_get_state(mbavo_vo *vo, mbavo_vo_state *st)
    {
        if (!vo || !st) return MBAVO_E_ARG;
        VO::TrackerState s;
        vo->impl.getState(s);
        memcpy(st, &s, sizeof(s));
        return 0;
    }

    int mbavo_vo_set_state(mbavo_vo *vo, const mbavo_vo_state *st)
    {
        if (!vo || !st) return MBAVO_E_ARG;
        VO::TrackerState s;
        memcpy(&s, st, sizeof(s));
        return vo->impl.setState(s);
    }

    int mbavo_vo_set_keyframe(mbavo_vo *vo, const unsigned char *sharp, const float *depth_z, double sharp_cap)
    {
        if (!vo || !sharp || !depth_z) return MBAVO_E_ARG;
        VO::FrameView s{sharp, sharp_cap, 0.0};
        return vo->impl.setKeyframe(s, depth_z);
    }

    int mbavo_vo_num_keypoints(mbavo_vo *vo, int level)
    {
        if (!vo || level < 0 || level >= vo->impl.getOptions().num_pyramid_levels) return MBAVO_E_ARG;
        return vo->impl.numKeypoints(level);
    }

    int mbavo_vo_get_keypoints(mbavo_vo *vo, int level, double *xy, double *z)
    {
        if (!vo || level < 0 || level >= vo->impl.getOptions().num_pyramid_levels || !xy || !z) return MBAVO_E_ARG;
        const int K = vo->impl.numKeypoints(level);
        if (K == 0) return 0;
        hipError_t e = hipMemcpy(xy, vo->impl.deviceKeypointsXY(level), sizeof(double) * 2 * K, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(z, vo->impl.deviceKeypointsZ(level), sizeof(double) * K, hipMemcpyDeviceToHost);
        return (int)e;
    }

    int mbavo_vo_track_frame(mbavo_vo *vo, const unsigned char *sharp, const float *depth_z, double sharp_cap,
                             const unsigned char *blur, double blur_cap, double blur_exp, double T_out[7], mbavo_vo_info *info)
    {
        if (!vo || !T_out) return MBAVO_E_ARG;
        VO::FrameView s{sharp, sharp_cap, 0.0}, b{blur, blur_cap, blur_exp};
        Core::Transformation T;
        VO::TrackInfo ti;
        const int rc = vo->impl.trackFrame(s, b, depth_z, &T, &ti);
        if (rc != 0) return rc;
        memcpy(T_out, T.getData(), sizeof(double) * 7);
        if (info)
        {
            info->is_keyframe = ti.is_keyframe; info->num_keypoints0 = ti.num_keypoints0; info->num_trace = ti.num_trace;
            info->start_idx = ti.start_idx; info->avg_flow = ti.avg_flow; info->avg_kernel = ti.avg_kernel;
            info->final_cost = ti.final_cost;
        }
        return 0;
    }

    int mbavo_p2p_create(mbavo_ctx *ctx, int rank, int world, long long max_doubles_per_slot, unsigned char *handle_out)
    {
        if (!ctx) return MBAVO_E_ARG;
        return ctx->engine->p2p_create(rank, world, max_doubles_per_slot, handle_out);
    }
    int mbavo_p2p_connect(mbavo_ctx *ctx, const unsigned char *all_handles) { return ctx ? ctx->engine->p2p_connect(all_handles) : MBAVO_E_ARG; }
    int mbavo_p2p_ranks(mbavo_ctx *ctx) { return ctx ? ctx->engine->p2p_ranks() : 0; }
    int mbavo_allgather_blocks_p2p(mbavo_ctx *ctx, double *d, long long count_per_rank)
    {
        return ctx ? ctx->engine->p2p_collective(0, d, count_per_rank) : MBAVO_E_ARG;
    }
    int mbavo_allreduce_blocks_p2p(mbavo_ctx *ctx, double *d, long long count) { return ctx ? ctx->engine->p2p_collective(1, d, count) : MBAVO_E_ARG; }
    int mbavo_p2p_status(mbavo_ctx *ctx) { return ctx ? ctx->engine->p2p_status() : MBAVO_E_ARG; }
    int mbavo_p2p_set_timeout(mbavo_ctx *ctx, double seconds) { return ctx ? ctx->engine->p2p_set_timeout(seconds) : MBAVO_E_ARG; }
    int mbavo_p2p_disconnect(mbavo_ctx *ctx) { return ctx ? ctx->engine->p2p_disconnect() : MBAVO_E_ARG; }
    int mbavo_p2p_destroy(mbavo_ctx *ctx) { return ctx ? ctx->engine->p2p_destroy() : MBAVO_E_ARG; }

    int mbavo_profile(mbavo_ctx *ctx, int enable)
    {
        if (!ctx) return MBAVO_E_ARG;
        ctx->engine->profile_enable(enable);
        return 0;
    }

    int mbavo_profile_read(mbavo_ctx *ctx, double *ms, int *n)
    {
        if (!ctx) return MBAVO_E_ARG;
        return ctx->engine->profile_read(ms, n);
    }

    void mbavo_timing_report(void) { mbavo::PhaseTimers::get().report(); }
    void mbavo_reload_env(void) { mbavo::reload_env_overrides(); }
    void mbavo_ride_along_stats(long long out[3])
    {
        mbavo::RideAlongStats &s = mbavo::RideAlongStats::get();
        out[0] = s.posts.exchange(0);
        out[1] = s.hits.exchange(0);
        out[2] = s.waits.exchange(0);
    }

    const char *mbavo_last_kernel(mbavo_ctx *ctx) { return ctx ? ctx->engine->last_kernel() : ""; }
    int mbavo_last_layout(mbavo_ctx *ctx, int out[8])
    {
        if (!ctx || !out) return MBAVO_E_ARG;
        ctx->engine->last_layout(out);
        return 0;
    }

    // ---- multi-GPU (multi_gpu.hip)
    int mbavo_shard_keypoints(const mbavo_problem *whole, int rank, int world, mbavo_problem *shard, int *first)
    {
        return mbavo::shard_keypoints(whole, rank, world, shard, first);
    }

    int mbavo_shard_frames(const mbavo_problem *whole, int rank, int world, mbavo_problem *shard, int *first)
    {
        return mbavo::shard_frames(whole, rank, world, shard, first);
    }

    int mbavo_system_len(int N) { return 1 + 6 * N + 36 * N * N; }

    int mbavo_merge_device(mbavo_ctx *ctx, int B, const mbavo_problem *probs, int k, const double *d_fb, double *d_systems)
    {
        if (!ctx) return MBAVO_E_ARG;
        return ctx->engine->merge_device(B, probs, k, d_fb, d_systems);
    }

    int mbavo_comm_unique_id(unsigned char *id) { return id ? mbavo::comm_unique_id(id) : MBAVO_E_ARG; }

    int mbavo_comm_init(mbavo_ctx *ctx, const unsigned char *id, int rank, int world)
    {
        if (!ctx || !id || world < 1 || rank < 0 || rank >= world) return MBAVO_E_ARG;
        return ctx->engine->comm_init(id, rank, world);
    }

    int mbavo_comm_ranks(mbavo_ctx *ctx) { return ctx ? ctx->engine->comm_ranks() : 0; }

    int mbavo_comm_destroy(mbavo_ctx *ctx) { return ctx ? ctx->engine->comm_destroy() : MBAVO_E_ARG; }

    int mbavo_allreduce_blocks(mbavo_ctx *ctx, void *comm, double *d_blocks, long long count)
    {
        if (!ctx || !d_blocks || count < 0) return MBAVO_E_ARG;
        return ctx->engine->allreduce(comm, d_blocks, d_blocks, count);
    }

    int mbavo_allreduce_blocks_to(mbavo_ctx *ctx, void *comm, const double *d_send, double *d_recv, long long count)
    {
        if (!ctx || !d_send || !d_recv || count < 0) return MBAVO_E_ARG;
        return ctx->engine->allreduce(comm, d_send, d_recv, count);
    }

    int mbavo_allgather_blocks(mbavo_ctx *ctx, void *comm, double *d_blocks, long long count_per_rank)
    {
        if (!ctx || !d_blocks || count_per_rank < 0) return MBAVO_E_ARG;
        return ctx->engine->allgather(comm, d_blocks, count_per_rank);
    }
}
