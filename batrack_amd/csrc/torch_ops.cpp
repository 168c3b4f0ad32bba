// torch_ops.cpp — torch.ops.batrack_hip.*: the operator registration the north star asks for, laid over the C ABI of
// include/batrack_ba.h (nothing is computed here).  The reference itself has no torch.ops registrations:
// its boundary is the Python function BA_rgbd_droid (/root/reference/main/backend/ba.py:217), which
// batrack_amd/backend/ba.py implements on top of these operators.  Every operator takes the plan as an integer handle
// (the bt_plan pointer), checks device / dtype / contiguity, fetches PyTorch's CURRENT HIP stream and calls the C entry
// point: no allocation, no synchronisation.
//   batrack_hip::plan_create(Tensor ii, Tensor jj, Tensor kk, int n_buf, int p_tot, int fixedp, int own_lo, int own_hi) -> int
//   batrack_hip::plan_destroy(int plan) -> ()
//   batrack_hip::plan_info(int plan) -> int[]                 (the fields of bt_plan_info, in order)
//   batrack_hip::ba_step(int plan, Tensor ws, Tensor poses, Tensor patches, Tensor mono, int mono_stride, Tensor intrinsics,
//                        Tensor targets, int target_stride, Tensor weights, Tensor poses_out, Tensor patches_out,
//                        float[] bounds, float lmbda, float ep, float alpha, int loss, bool structure_only, int phase,
//                        Tensor? lmbda_per_track=None) -> int
//       phase 0 = the whole step, 1 = bt_ba_reduce, 2 = bt_ba_pack, 3 = bt_ba_unpack, 4 = bt_ba_solve_update
//   batrack_hip::ba_droid(int plan, Tensor ws, Tensor poses, Tensor patches, Tensor patches_monodisp, Tensor intrinsics,
//                         Tensor targets_2d, Tensor weights, float[] bounds, float lmbda, float ep, float alpha, int loss,
//                         bool structure_only, Tensor? lmbda_per_track=None) -> (Tensor, Tensor)
//       one BA_rgbd_droid call with the caller's tensors as they are (ba.py:217-339: poses [1, N, 7], patches [1, P, 3, 1, 1],
//       the prior and the 2-D targets possibly strided views): shape checks, the views the ABI needs, the two output
//       tensors and the step in one operator call — the Python wrapper's dozen tensor operations cost more host time
//       (28 us a call) than a structure-only step takes on the GPU (9 us)
//   batrack_hip::world_tracks(Tensor poses, Tensor patches, Tensor intrinsics, Tensor ix, Tensor(a!) patches_local,
//                             Tensor local_weights, int m, Tensor(b!)? points=None, Tensor(c!)? world=None) -> ()
//       bt_world_tracks (include/batrack_projective.h): poses [N, 7], patches [N*M, 3, p, p], intrinsics [N, 4], ix int64,
//       patches_local [N*M, S_local, 3] in/out, local_weights [N*M, S_local], points [>= m, 3], world [N*M, S_local, 3]
//   batrack_hip::corr_pyramid(Tensor fmaps, int levels) -> Tensor
//       bt_corr_pyramid (include/batrack_corr.h): fmaps [..., C, H, W] -> the packed channels-last pyramid, one 1-D tensor
//   batrack_hip::corr_lookup(Tensor pyramid, int[] shape, int levels, int radius, Tensor targets, Tensor coords) -> Tensor
//       bt_corr_lookup: shape = [S', C, H, W] of the maps the pyramid was made from, targets [..., N, C], coords [..., N, 2]
//       (the strided view `coords3[..., :2]` is read in place) -> [..., N, levels * (2 radius + 1)^2]
//   batrack_hip::observe_window(Tensor traj, Tensor depth, Tensor vis, Tensor dyn, Tensor queries, Tensor? dmaps, Tensor ii, Tensor jj,
//                               Tensor kk, Tensor(a!) patches_valid, Tensor(b!) patches_local, Tensor(c!)? local_monodisp,
//                               Tensor(d!)? local_vis, Tensor(e!)? local_static, Tensor(f!)? local_weights, Tensor(g!) workspace,
//                               int n, int Sp, int kf_stride, int H, int W, float wd, float ht, int padding, float? vis_threshold,
//                               float static_quantile, float static_threshold, int min_track_len, bool is_initialized,
//                               int interp_w, int interp_h) -> (Tensor, Tensor, Tensor, Tensor)
//       bt_observe_window (include/batrack_observe.h): traj [S, Nq, 2], depth / vis / dyn [S, Nq], queries [Nq, 3], dmaps [Sp, H, W],
//       ii / jj / kk [Nq*Sp] int64, patches_valid [N, M], patches_local [N*M, S_local, 3], the other window buffers [N*M, S_local],
//       workspace: bt_observe_workspace_bytes() bytes -> targets_3d [E, 3], weights [E, 2], weights_pose [E, 2], query_disp [Nq]
//       (query_disp is empty without dmaps)
//   batrack_hip::track_pos_embed(Tensor tabx, Tensor taby, Tensor coords) -> Tensor
//       bt_track_pos_embed (include/batrack_track.h): tabx [W, E/2], taby [H, E/2], coords [N, >= 2] with unit last stride
//       (a row view of the tracker's [S, N, 3] state is read in place) -> [N, E]
//   batrack_hip::track_tokens(Tensor coords, Tensor? coords_sub, Tensor fcorrs, Tensor ffeats, Tensor track_mask, Tensor vis,
//                             Tensor pos, Tensor time, Tensor w_flow, Tensor b_flow, bool fix_track_mask) -> Tensor
//       bt_track_tokens: coords [S, N, 3], fcorrs [S, N, LRR], ffeats [S, N, C], track_mask / vis [S, N], pos [N, E], time [S, E],
//       w_flow [F, 195], b_flow [F], all contiguous -> x [N, S, E], E = F + LRR + C + 2
//   batrack_hip::track_apply(Tensor delta, Tensor gamma, Tensor beta, Tensor w_u, Tensor b_u, Tensor(a!) state, Tensor(b!) ffeats,
//                            Tensor? total, Tensor? dyn_mask, float stride, float dz, float d_range, float d_near,
//                            bool use_log_depth) -> Tensor
//       bt_track_apply: delta [N, S, 3 + C]; state [S, N, 3] and ffeats [S, N, C] updated in place; total [S, N, 3] and
//       dyn_mask [N] select the static pass -> out [S, N, 3]
//   batrack_hip::attention(Tensor qkv, int heads, int n_seq, int L, int seq_stride, int tok_stride, float scale) -> Tensor
//       bt_attention (include/batrack_attn.h): qkv [rows, >= 3 * heads * 48] with unit last stride (the row stride is read from
//       the tensor); token i of sequence b is row b * seq_stride + i * tok_stride -> [rows, heads * 48] (rows that no token
//       addresses are left unwritten)
//   batrack_hip::rows_linear(Tensor x, Tensor w_hi, Tensor w_lo, float inv_scale, Tensor? bias, float norm_eps, bool gelu,
//                            Tensor? residual, Tensor(a!) out, int precision) -> ()
//       bt_rows_linear (include/batrack_rows.h): x [rows, K] and out, residual [rows, Nout] with unit last stride (the row
//       strides are read from the tensors); w_hi, w_lo [Nout, K] float16 contiguous; norm_eps < 0: no LayerNorm prologue
//   batrack_hip::depth_range(Tensor depth, bool use_log_depth) -> Tensor
//       bt_depth_range (include/batrack_window.h): depth [T, H, W], any strides (read in place) -> [2] (min, max) on the device
//   batrack_hip::window_depth(Tensor depth, int S, int stride, float d_near, float d_range, float dz, bool use_log_depth) -> (Tensor, Tensor)
//       bt_window_depth: depth [frames <= S, H, W], any strides -> dmaps [S, H / stride, W / stride] and zrange [2]
//   batrack_hip::embed_conv(Tensor fnet_maps, Tensor dmaps, Tensor zrange, Tensor wpacked, Tensor bias, Tensor freqs, int frame0,
//                           Tensor(a!) out) -> ()
//       bt_embed_conv: fnet_maps [F, 128, h, w], any strides; dmaps [S, h, w]; wpacked [24, 9, 8, 128]; out [F, 128, h, w] contiguous
//   batrack_hip::feat_sample(Tensor fmaps, Tensor frames, Tensor xy) -> Tensor
//       bt_feat_sample: fmaps [S, 128, h, w] contiguous, frames [n] int32, xy [n, >= 2] with unit last stride -> [n, 128]
//   batrack_hip::encoder_head(Tensor a, Tensor b, Tensor c, Tensor d, Tensor w2_packed, Tensor bias2, Tensor w3_packed, Tensor bias3,
//                             Tensor(a!) out) -> ()
//       bt_encoder_head (include/batrack_encoder.h): the levels [F, 64 / 96 / 128 / 128, h_l, w_l], any strides; w2_packed
//       [52, 9, 8, 256]; w3_packed [256, 128]; out [F, 128, h, w] contiguous, whose h and w are the output map's
//   batrack_hip::res_block(Tensor x, Tensor w1, Tensor b1, Tensor w2, Tensor b2, Tensor? wd, Tensor? bd, int stride, Tensor(a!) out) -> ()
//       bt_res_block (include/batrack_encoder.h): x [F, c_in, h, w], any strides; w1 [c_in / 8, 9, 8, c_out]; w2 [c_out / 8, 9, 8,
//       c_out]; wd [c_in, c_out] and bd exactly when stride is 2; out [F, c_out, ho, wo] contiguous
//   batrack_hip::encoder_stem(Tensor x, Tensor w, Tensor b, Tensor(a!) out) -> ()
//       bt_encoder_stem (include/batrack_encoder.h): x [F, 3, h, w], any strides; w [7, 3, 8, 64]; out [F, 64, ho, wo] contiguous
//   batrack_hip::frame_prep(Tensor image, Tensor depth, bool normalise, bool use_log_depth, Tensor(a!) workspace, Tensor(b!) rgbd,
//                           Tensor(c!) drange) -> ()
//       bt_frame_prep (include/batrack_video.h): image [F, 3, H, W] uint8 or float32, any strides (a permuted HWC view is read in
//       place); depth [F, H, W] float32, any strides; workspace int32, at least bt_frame_prep_workspace_bytes(F, oh, ow) bytes, its
//       tickets zero (the kernel leaves them zero: one workspace serves every call of a stream); rgbd [F, 4, oh, ow] contiguous, whose
//       oh and ow are the output size; drange [F, 2].  One launch, nothing allocated.
// Built by batrack_amd/_lib.py:build() into batrack_amd/lib/libbatrack_torch.so (g++, host code only).
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <tuple>
#include <vector>

#include "../../include/batrack_attn.h"
#include "../../include/batrack_ba.h"
#include "../../include/batrack_corr.h"
#include "../../include/batrack_encoder.h"
#include "../../include/batrack_observe.h"
#include "../../include/batrack_projective.h"
#include "../../include/batrack_rows.h"
#include "../../include/batrack_track.h"
#include "../../include/batrack_video.h"
#include "../../include/batrack_window.h"

namespace {

const float *f32(const at::Tensor &t, const char *what) {
    TORCH_CHECK(t.is_cuda(), "batrack_hip: `", what, "` must be on the GPU (no CPU fallback)");
    TORCH_CHECK(t.scalar_type() == at::kFloat, "batrack_hip: `", what, "` must be float32");
    return t.data_ptr<float>();
}

// every tensor is float32 on the GPU of the first (and contiguous, where the operator reads none in place)
void all_f32(const char *op, const std::vector<const at::Tensor *> &ts, bool contiguous = false) {
    for (const at::Tensor *t : ts) {
        (void)f32(*t, "an argument");
        TORCH_CHECK((!contiguous || t->is_contiguous()) && t->device() == ts[0]->device(), op,
                    contiguous ? "tensors must be contiguous and on one device" : "tensors must be on one device");
    }
}

bt_encoder_level level_of(const at::Tensor &t) {                 // a 4-D float32 tensor as the strided view it is
    return bt_encoder_level{t.data_ptr<float>(), t.size(1), t.size(2), t.size(3), t.stride(0), t.stride(1), t.stride(2), t.stride(3)};
}

at::Tensor scratch(size_t bytes, const at::Tensor &like) {       // on `like`'s device; needs no initialisation
    return at::empty({(int64_t)((bytes + 7) / 8)}, like.options().dtype(at::kDouble));
}

int64_t plan_create(const at::Tensor &ii, const at::Tensor &jj, const at::Tensor &kk, int64_t n_buf, int64_t p_tot,
                    int64_t fixedp, int64_t own_lo, int64_t own_hi) {
    for (const at::Tensor *t : {&ii, &jj, &kk})
        TORCH_CHECK(t->scalar_type() == at::kLong && t->is_contiguous() && t->numel() == ii.numel(),
                    "batrack_hip::plan_create: indices must be contiguous int64 of one length (batrack.py:100-102)");
    if (ii.is_cuda()) c10::hip::getCurrentHIPStream(ii.device().index()).synchronize();   // the indices must be complete
    bt_plan *plan = nullptr;
    const int rc = bt_plan_create(ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(), kk.data_ptr<int64_t>(), ii.numel(), n_buf, p_tot,
                                  fixedp, 0, own_lo, own_hi, ii.is_cuda() ? 1 : 0, 1, &plan);
    TORCH_CHECK(rc == BT_OK, "batrack_hip::plan_create failed with status ", rc, rc == BT_EUNSUPPORTED ?
                " (unsupported graph: more than 255 free poses, a track seen by more than 64 free cameras, or edges of one "
                "track naming different source frames)" : "");
    return reinterpret_cast<int64_t>(plan);
}

void plan_destroy(int64_t plan) { bt_plan_destroy(reinterpret_cast<bt_plan *>(plan)); }

std::vector<int64_t> plan_info(int64_t plan) {
    bt_plan_info I{};
    TORCH_CHECK(bt_plan_get_info(reinterpret_cast<const bt_plan *>(plan), &I) == BT_OK, "batrack_hip::plan_info: bad handle");
    return {I.E, I.n_buf, I.p_tot, I.fixedp, I.n_all, I.n, I.m, I.pairs, I.tiles, I.slots, I.erows, I.max_tile_cams,
            I.nnz_blocks, I.updates, I.workspace_bytes, I.sorted_input};
}

int64_t ba_step(int64_t plan, const at::Tensor &ws, const at::Tensor &poses, const at::Tensor &patches, const at::Tensor &mono,
                int64_t mono_stride, const at::Tensor &intrinsics, const at::Tensor &targets, int64_t target_stride,
                const at::Tensor &weights, const at::Tensor &poses_out, const at::Tensor &patches_out, c10::ArrayRef<double> bounds,
                double lmbda, double ep, double alpha, int64_t loss, bool structure_only, int64_t phase,
                const c10::optional<at::Tensor> &lmbda_per_track) {
    TORCH_CHECK(bounds.size() == 4, "batrack_hip::ba_step: bounds = [x0, y0, x1, y1]");
    TORCH_CHECK(ws.is_cuda() && ws.is_contiguous(), "batrack_hip::ba_step: the workspace must be a contiguous GPU tensor");
    bt_ba_args a{};
    a.poses = f32(poses, "poses"); a.patches = f32(patches, "patches"); a.mono_disp = f32(mono, "mono_disp");
    a.intrinsics = f32(intrinsics, "intrinsics"); a.targets = f32(targets, "targets"); a.weights = f32(weights, "weights");
    a.target_stride = target_stride; a.mono_stride = mono_stride;
    a.poses_out = const_cast<float *>(f32(poses_out, "poses_out")); a.patches_out = const_cast<float *>(f32(patches_out, "patches_out"));
    for (int i = 0; i < 4; ++i) a.bounds[i] = (float)bounds[i];
    a.lmbda_per_track = lmbda_per_track.has_value() ? f32(*lmbda_per_track, "lmbda_per_track") : nullptr;
    if (lmbda_per_track.has_value()) TORCH_CHECK(lmbda_per_track->is_contiguous(), "batrack_hip::ba_step: lmbda_per_track must be contiguous");
    a.lmbda = (float)lmbda; a.ep = (float)ep; a.alpha = (float)alpha; a.loss = (int32_t)loss; a.structure_only = structure_only ? 1 : 0;
    const bt_plan *p = reinterpret_cast<const bt_plan *>(plan);
    void *st = c10::hip::getCurrentHIPStream(ws.device().index()).stream();
    int rc;
    switch (phase) {
        case 0: rc = bt_ba_step(p, &a, ws.data_ptr(), st); break;
        case 1: rc = bt_ba_reduce(p, &a, ws.data_ptr(), st); break;
        case 2: rc = bt_ba_pack(p, &a, ws.data_ptr(), st); break;
        case 3: rc = bt_ba_unpack(p, &a, ws.data_ptr(), st); break;
        case 4: rc = bt_ba_solve_update(p, &a, ws.data_ptr(), st); break;
        default: rc = BT_EINVAL;
    }
    return rc;
}

std::tuple<at::Tensor, at::Tensor> ba_droid(int64_t plan, const at::Tensor &ws, const at::Tensor &poses, const at::Tensor &patches,
                                             const at::Tensor &monodisp, const at::Tensor &intrinsics, const at::Tensor &targets_2d,
                                             const at::Tensor &weights, c10::ArrayRef<double> bounds, double lmbda, double ep, double alpha,
                                             int64_t loss, bool structure_only, const c10::optional<at::Tensor> &lmbda_per_track) {
    const bt_plan *p = reinterpret_cast<const bt_plan *>(plan);
    bt_plan_info I{};
    TORCH_CHECK(bt_plan_get_info(p, &I) == BT_OK, "batrack_hip::ba_droid: bad plan handle");
    TORCH_CHECK(poses.dim() == 3 && poses.size(0) == 1 && poses.size(2) == 7 && poses.size(1) == I.n_buf,
                "poses must wrap a [1, N, 7] tensor of the plan's N pose slots (batch b = 1, ba.py:218)");
    TORCH_CHECK(patches.dim() >= 3 && patches.size(0) == 1 && patches.size(2) == 3 && patches.numel() == 3 * I.p_tot,
                "patches must be [1, P_tot, 3, 1, 1] with the plan's P_tot (patch size 1, batrack.py:45)");
    const int64_t n_buf = I.n_buf, p_tot = I.p_tot, E = I.E;
    const at::Tensor Pc = poses.contiguous(), pat = patches.reshape({p_tot, 3}).contiguous();
    (void)f32(Pc, "poses"); (void)f32(pat, "patches");
    // the caller's prior is a strided view (patches_local[:, :, mid, 2:], batrack.py:866): used in place through mono_stride —
    // only a genuine stride >= 1 (an expanded tensor, stride 0, or a negative stride is materialised)
    at::Tensor mono = monodisp;
    TORCH_CHECK(mono.numel() == p_tot, "patches_monodisp does not match the patch buffer");
    int64_t mstride = 1;
    if (!mono.is_contiguous() && p_tot > 1) {
        int64_t d = -1, nd = 0;
        for (int64_t k = 0; k < mono.dim(); ++k) if (mono.size(k) == p_tot) { d = k; ++nd; }
        if (nd == 1 && mono.stride(d) >= 1) { mstride = mono.stride(d); mono = mono.as_strided({p_tot}, {mstride}, mono.storage_offset()); }
        else mono = mono.reshape({-1}).contiguous();
    } else mono = mono.reshape({-1});
    const at::Tensor intr = intrinsics.reshape({-1, 4}).contiguous();
    TORCH_CHECK(intr.size(0) == n_buf, "intrinsics do not match the pose buffer");
    TORCH_CHECK(targets_2d.size(-1) == 2 && targets_2d.numel() == 2 * E, "targets_2d must be [1, E, 2]");
    at::Tensor tg = targets_2d.is_contiguous() ? targets_2d.reshape({E, 2}) : targets_2d.select(0, 0);     // the caller's view has strides (3, 1): used in place
    if (tg.dim() != 2 || tg.stride(1) != 1) tg = targets_2d.reshape({E, 2}).contiguous();
    const at::Tensor w = weights.reshape({E, 2}).contiguous();
    at::Tensor patches_out = at::empty_like(pat), poses_out = structure_only ? Pc : at::empty_like(Pc);
    bt_ba_args a{};
    a.poses = Pc.data_ptr<float>(); a.patches = pat.data_ptr<float>(); a.mono_disp = f32(mono, "patches_monodisp");
    a.intrinsics = f32(intr, "intrinsics"); a.targets = f32(tg, "targets_2d"); a.weights = f32(w, "weights");
    a.target_stride = tg.stride(0); a.mono_stride = mstride;
    a.poses_out = poses_out.data_ptr<float>(); a.patches_out = patches_out.data_ptr<float>();
    TORCH_CHECK(bounds.size() == 4, "bounds = [x0, y0, x1, y1]");
    for (int i = 0; i < 4; ++i) a.bounds[i] = (float)bounds[i];
    if (lmbda_per_track.has_value()) {
        TORCH_CHECK(lmbda_per_track->is_contiguous() && lmbda_per_track->numel() == I.m, "a lmbda tensor must hold one value per distinct track (ba.py:299-300)");
        a.lmbda_per_track = f32(*lmbda_per_track, "lmbda");
    }
    a.lmbda = (float)lmbda; a.ep = (float)ep; a.alpha = (float)alpha; a.loss = (int32_t)loss; a.structure_only = structure_only ? 1 : 0;
    TORCH_CHECK(ws.is_cuda() && ws.is_contiguous(), "batrack_hip::ba_droid: the workspace must be a contiguous GPU tensor");
    const int rc = bt_ba_step(p, &a, ws.data_ptr(), c10::hip::getCurrentHIPStream(ws.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, "batrack_hip::ba_droid: bt_ba_step failed with status ", rc);
    return {poses_out, patches_out.view({1, p_tot, 3, 1, 1})};
}

void world_tracks(const at::Tensor &poses, const at::Tensor &patches, const at::Tensor &intrinsics, const at::Tensor &ix,
                  const at::Tensor &patches_local, const at::Tensor &local_weights, int64_t m, const c10::optional<at::Tensor> &points,
                  const c10::optional<at::Tensor> &world) {
    const char *op = "batrack_hip::world_tracks: ";
    const float *P = f32(poses, "poses"), *pat = f32(patches, "patches"), *K = f32(intrinsics, "intrinsics");
    float *pl = const_cast<float *>(f32(patches_local, "patches_local"));
    const float *lw = f32(local_weights, "local_weights");
    TORCH_CHECK(ix.is_cuda() && ix.scalar_type() == at::kLong && ix.is_contiguous(), op, "`ix` must be a contiguous int64 GPU tensor");
    for (const at::Tensor *t : {&poses, &patches, &intrinsics, &patches_local, &local_weights})
        TORCH_CHECK(t->is_contiguous() && t->device() == poses.device(), op, "tensors must be contiguous and on one device");
    TORCH_CHECK(ix.device() == poses.device(), op, "tensors must be on one device");
    TORCH_CHECK(poses.dim() == 2 && poses.size(1) == 7, op, "poses must be [N, 7]");
    const int64_t N = poses.size(0);
    TORCH_CHECK(intrinsics.dim() == 2 && intrinsics.size(0) == N && intrinsics.size(1) == 4, op, "intrinsics must be [N, 4]");
    TORCH_CHECK(patches.dim() == 4 && patches.size(1) == 3 && patches.size(2) == patches.size(3), op, "patches must be [N*M, 3, p, p]");
    const int64_t NM = patches.size(0);
    TORCH_CHECK(patches_local.dim() == 3 && patches_local.size(0) == NM && patches_local.size(2) == 3, op,
                "patches_local must be [N*M, S_local, 3] over the patch buffer");
    const int64_t S = patches_local.size(1);
    TORCH_CHECK(local_weights.numel() == NM * S, op, "local_weights must be [N*M, S_local]");
    TORCH_CHECK(m >= 0 && m <= NM && ix.numel() >= m, op, "m tracks must fit the patch buffer and `ix`");
    float *pts = nullptr, *wld = nullptr;
    if (points.has_value()) {
        TORCH_CHECK(points->is_contiguous() && points->device() == poses.device() && points->numel() >= 3 * m, op,
                    "points must be a contiguous [>= m, 3] tensor");
        pts = const_cast<float *>(f32(*points, "points"));
    }
    if (world.has_value()) {
        TORCH_CHECK(world->is_contiguous() && world->device() == poses.device() && world->numel() == NM * S * 3, op,
                    "world must be a contiguous [N*M, S_local, 3] tensor");
        wld = const_cast<float *>(f32(*world, "world"));
    }
    const int rc = bt_world_tracks(P, N, K, pat, NM, patches.size(2) * patches.size(3), ix.data_ptr<int64_t>(), pl, lw, S, m, pts, wld,
                                   c10::hip::getCurrentHIPStream(poses.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_world_tracks failed with status ", rc);
}

at::Tensor corr_pyramid(const at::Tensor &fmaps, int64_t levels) {
    const char *op = "batrack_hip::corr_pyramid: ";
    (void)f32(fmaps, "fmaps");
    TORCH_CHECK(fmaps.dim() >= 4 && fmaps.is_contiguous(), op, "fmaps must be a contiguous [..., C, H, W] tensor");
    const int64_t n = fmaps.dim(), C = fmaps.size(n - 3), H = fmaps.size(n - 2), W = fmaps.size(n - 1);
    const int64_t S = C * H * W > 0 ? fmaps.numel() / (C * H * W) : 0;
    const size_t bytes = bt_corr_pyramid_bytes(S, C, H, W, (int32_t)levels);
    at::Tensor pyr = at::empty({(int64_t)(bytes / sizeof(float))}, fmaps.options());
    const int rc = bt_corr_pyramid(fmaps.data_ptr<float>(), S, C, H, W, (int32_t)levels, pyr.data_ptr<float>(),
                                   c10::hip::getCurrentHIPStream(fmaps.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_corr_pyramid failed with status ", rc);
    return pyr;
}

at::Tensor corr_lookup(const at::Tensor &pyramid, c10::ArrayRef<int64_t> shape, int64_t levels, int64_t radius,
                       const at::Tensor &targets, const at::Tensor &coords) {
    const char *op = "batrack_hip::corr_lookup: ";
    const float *pyr = f32(pyramid, "pyramid"), *tg = f32(targets, "targets");
    (void)f32(coords, "coords");
    TORCH_CHECK(shape.size() == 4, op, "shape = [S', C, H, W] of the feature maps");
    const int64_t S = shape[0], C = shape[1], H = shape[2], W = shape[3];
    TORCH_CHECK(pyramid.is_contiguous() && pyramid.numel() * sizeof(float) == bt_corr_pyramid_bytes(S, C, H, W, (int32_t)levels)
                && pyramid.numel() > 0, op, "`pyramid` is not the pyramid of maps of this shape and level count");
    TORCH_CHECK(targets.dim() >= 2 && targets.is_contiguous() && targets.size(-1) == C, op, "targets must be contiguous [..., N, C]");
    const int64_t N = targets.size(-2);
    TORCH_CHECK(targets.numel() == S * N * C, op, "targets must hold S' * N vectors");
    TORCH_CHECK(coords.dim() == targets.dim() && coords.size(-1) == 2 && coords.numel() == S * N * 2, op, "coords must be [..., N, 2]");
    TORCH_CHECK(targets.device() == pyramid.device() && coords.device() == pyramid.device(), op, "tensors must be on one device");
    // (x, y) pairs a constant number of floats apart are read in place: a contiguous tensor (2) or a `[..., :2]` view (3)
    at::Tensor cd = coords;
    int64_t cs = cd.stride(-2);
    bool flat = cd.stride(-1) == 1 && cs >= 2;
    for (int64_t k = cd.dim() - 3, run = cs * N; flat && k >= 0; run *= cd.size(k), --k)
        flat = cd.size(k) == 1 || cd.stride(k) == run;
    if (!flat || S * N <= 1) { cd = coords.contiguous(); cs = 2; }
    std::vector<int64_t> osz(coords.sizes().begin(), coords.sizes().end());
    const int64_t d = 2 * radius + 1;
    osz.back() = levels * d * d;
    at::Tensor out = at::empty(osz, targets.options());
    if (N == 0) return out;
    const int rc = bt_corr_lookup(pyr, S, C, H, W, (int32_t)levels, (int32_t)radius, tg, cd.data_ptr<float>(), cs, N, out.data_ptr<float>(),
                                  c10::hip::getCurrentHIPStream(pyramid.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_corr_lookup failed with status ", rc);
    return out;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> observe_window(
        const at::Tensor &traj, const at::Tensor &depth, const at::Tensor &vis, const at::Tensor &dyn, const at::Tensor &queries,
        const c10::optional<at::Tensor> &dmaps, const at::Tensor &ii, const at::Tensor &jj, const at::Tensor &kk,
        const at::Tensor &patches_valid, const at::Tensor &patches_local, const c10::optional<at::Tensor> &local_monodisp,
        const c10::optional<at::Tensor> &local_vis, const c10::optional<at::Tensor> &local_static,
        const c10::optional<at::Tensor> &local_weights, const at::Tensor &workspace, int64_t n, int64_t Sp, int64_t kf_stride, int64_t H,
        int64_t W, double wd, double ht, int64_t padding, c10::optional<double> vis_threshold, double static_quantile,
        double static_threshold, int64_t min_track_len, bool is_initialized, int64_t interp_w, int64_t interp_h) {
    const char *op = "batrack_hip::observe_window: ";
    bt_observe_args a{};
    a.traj = f32(traj, "traj"); a.depth = f32(depth, "depth"); a.vis = f32(vis, "vis"); a.dyn = f32(dyn, "dyn");
    a.queries = f32(queries, "queries");
    a.patches_valid = const_cast<float *>(f32(patches_valid, "patches_valid"));
    a.patches_local = const_cast<float *>(f32(patches_local, "patches_local"));
    const auto dev = traj.device();
    for (const at::Tensor *t : {&traj, &depth, &vis, &dyn, &queries, &patches_valid, &patches_local, &ii, &jj, &kk, &workspace})
        TORCH_CHECK(t->is_contiguous() && t->device() == dev, op, "tensors must be contiguous and on one device");
    TORCH_CHECK(traj.dim() == 3 && traj.size(2) == 2, op, "traj must be [S, Nq, 2]");
    const int64_t S = traj.size(0), Nq = traj.size(1);
    for (const at::Tensor *t : {&depth, &vis, &dyn})
        TORCH_CHECK(t->numel() == S * Nq, op, "depth, vis and dyn must be [S, Nq]");
    TORCH_CHECK(queries.numel() == 3 * Nq, op, "queries must be [Nq, 3]");
    TORCH_CHECK(Sp >= 0 && Sp <= S, op, "Sp frames of the window must fit its padded length S");
    const int64_t E = Nq * Sp;
    for (const at::Tensor *t : {&ii, &jj, &kk})
        TORCH_CHECK(t->scalar_type() == at::kLong && t->numel() == E, op, "ii, jj, kk must be int64 of Nq*Sp edges");
    TORCH_CHECK(patches_valid.dim() == 2, op, "patches_valid must be [N, M]");
    const int64_t N = patches_valid.size(0), M = patches_valid.size(1);
    TORCH_CHECK(patches_local.dim() == 3 && patches_local.size(0) == N * M && patches_local.size(2) == 3, op,
                "patches_local must be [N*M, S_local, 3]");
    const int64_t S_local = patches_local.size(1);
    float **opt[4] = {&a.local_monodisp, &a.local_vis, &a.local_static, &a.local_weights};
    const c10::optional<at::Tensor> *ot[4] = {&local_monodisp, &local_vis, &local_static, &local_weights};
    for (int i = 0; i < 4; ++i)
        if (ot[i]->has_value()) {
            const at::Tensor &t = **ot[i];
            TORCH_CHECK(t.is_contiguous() && t.device() == dev && t.numel() == N * M * S_local, op, "a window buffer must be contiguous [N*M, S_local]");
            *opt[i] = const_cast<float *>(f32(t, "window buffer"));
        }
    if (dmaps.has_value()) {
        TORCH_CHECK(dmaps->is_contiguous() && dmaps->device() == dev && dmaps->numel() == Sp * H * W, op, "dmaps must be contiguous [Sp, H, W]");
        a.dmaps = f32(*dmaps, "dmaps");
    }
    TORCH_CHECK(workspace.is_cuda() && workspace.numel() * workspace.element_size() >= (int64_t)bt_observe_workspace_bytes(), op,
                "the workspace is smaller than bt_observe_workspace_bytes()");
    at::Tensor targets = at::empty({E, 3}, traj.options()), weights = at::empty({E, 2}, traj.options()),
               weights_pose = at::empty({E, 2}, traj.options()), query_disp = at::empty({a.dmaps ? Nq : 0}, traj.options());
    a.targets_3d = targets.data_ptr<float>(); a.weights = weights.data_ptr<float>(); a.weights_pose = weights_pose.data_ptr<float>();
    a.query_disp = a.dmaps ? query_disp.data_ptr<float>() : nullptr;
    a.ii = ii.data_ptr<int64_t>(); a.jj = jj.data_ptr<int64_t>(); a.kk = kk.data_ptr<int64_t>();
    a.S = S; a.Sp = Sp; a.Nq = Nq; a.E = E; a.n = n; a.M = M; a.N = N; a.kf_stride = kf_stride; a.S_local = S_local; a.H = H; a.W = W;
    a.interp_w = interp_w; a.interp_h = interp_h; a.padding = padding; a.min_track_len = min_track_len;
    a.has_vis_threshold = vis_threshold.has_value() ? 1 : 0; a.is_initialized = is_initialized ? 1 : 0;
    a.wd = wd; a.ht = ht; a.vis_threshold = vis_threshold.value_or(0.0); a.static_quantile = static_quantile; a.static_threshold = static_threshold;
    const int rc = bt_observe_window(&a, workspace.data_ptr(), c10::hip::getCurrentHIPStream(dev.index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_observe_window failed with status ", rc);
    return {targets, weights, weights_pose, query_disp};
}

at::Tensor track_pos_embed(const at::Tensor &tabx, const at::Tensor &taby, const at::Tensor &coords) {
    const char *op = "batrack_hip::track_pos_embed: ";
    const float *tx = f32(tabx, "tabx"), *ty = f32(taby, "taby"), *cd = f32(coords, "coords");
    TORCH_CHECK(tabx.dim() == 2 && taby.dim() == 2 && tabx.is_contiguous() && taby.is_contiguous() && tabx.size(1) == taby.size(1),
                op, "tabx [W, E/2] and taby [H, E/2] must be contiguous");
    TORCH_CHECK(coords.dim() == 2 && coords.size(1) >= 2 && (coords.size(0) <= 1 || coords.stride(0) >= 2) && coords.stride(1) == 1,
                op, "coords must be [N, >= 2] with unit last stride");
    TORCH_CHECK(tabx.device() == coords.device() && taby.device() == coords.device(), op, "tensors must be on one device");
    const int64_t N = coords.size(0), E = 2 * tabx.size(1);
    at::Tensor out = at::empty({N, E}, tabx.options());
    if (N == 0) return out;
    const int rc = bt_track_pos_embed(tx, ty, taby.size(0), tabx.size(0), E, cd, N > 1 ? coords.stride(0) : 2, N, out.data_ptr<float>(),
                                      c10::hip::getCurrentHIPStream(coords.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_track_pos_embed failed with status ", rc);
    return out;
}

at::Tensor track_tokens(const at::Tensor &coords, const c10::optional<at::Tensor> &coords_sub, const at::Tensor &fcorrs,
                        const at::Tensor &ffeats, const at::Tensor &track_mask, const at::Tensor &vis, const at::Tensor &pos,
                        const at::Tensor &time, const at::Tensor &w_flow, const at::Tensor &b_flow, bool fix_track_mask) {
    const char *op = "batrack_hip::track_tokens: ";
    TORCH_CHECK(coords.dim() == 3 && coords.size(2) == 3 && fcorrs.dim() == 3 && ffeats.dim() == 3, op,
                "coords [S, N, 3], fcorrs [S, N, LRR], ffeats [S, N, C]");
    const int64_t S = coords.size(0), N = coords.size(1), LRR = fcorrs.size(2), C = ffeats.size(2);
    TORCH_CHECK(w_flow.dim() == 2 && w_flow.size(1) == BT_TRACK_EMB && b_flow.numel() == w_flow.size(0), op, "w_flow [F, 195], b_flow [F]");
    const int64_t F = w_flow.size(0), E = F + LRR + C + 2;
    all_f32(op, {&coords, &fcorrs, &ffeats, &track_mask, &vis, &pos, &time, &w_flow, &b_flow}, true);
    TORCH_CHECK(fcorrs.size(0) == S && fcorrs.size(1) == N && ffeats.size(0) == S && ffeats.size(1) == N && track_mask.numel() == S * N
                && vis.numel() == S * N && pos.numel() == N * E && time.numel() == S * E, op, "shapes disagree");
    const float *sub = nullptr;
    if (coords_sub.has_value()) {
        sub = f32(*coords_sub, "coords_sub");
        TORCH_CHECK(coords_sub->is_contiguous() && coords_sub->sizes() == coords.sizes() && coords_sub->device() == coords.device(), op,
                    "coords_sub must be like coords");
    }
    at::Tensor x = at::empty({N, S, E}, coords.options());
    if (N == 0) return x;
    const int rc = bt_track_tokens(coords.data_ptr<float>(), sub, fcorrs.data_ptr<float>(), ffeats.data_ptr<float>(),
                                   track_mask.data_ptr<float>(), vis.data_ptr<float>(), pos.data_ptr<float>(), time.data_ptr<float>(),
                                   w_flow.data_ptr<float>(), b_flow.data_ptr<float>(), S, N, F, LRR, C, fix_track_mask ? 1 : 0,
                                   x.data_ptr<float>(), c10::hip::getCurrentHIPStream(coords.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_track_tokens failed with status ", rc);
    return x;
}

at::Tensor track_apply(const at::Tensor &delta, const at::Tensor &gamma, const at::Tensor &beta, const at::Tensor &w_u,
                       const at::Tensor &b_u, at::Tensor state, at::Tensor ffeats, const c10::optional<at::Tensor> &total,
                       const c10::optional<at::Tensor> &dyn_mask, double stride, double dz, double d_range, double d_near,
                       bool use_log_depth) {
    const char *op = "batrack_hip::track_apply: ";
    TORCH_CHECK(delta.dim() == 3 && state.dim() == 3 && state.size(2) == 3 && ffeats.dim() == 3, op,
                "delta [N, S, 3 + C], state [S, N, 3], ffeats [S, N, C]");
    const int64_t N = delta.size(0), S = delta.size(1), C = ffeats.size(2);
    all_f32(op, {&delta, &gamma, &beta, &w_u, &b_u, &state, &ffeats}, true);
    TORCH_CHECK(delta.size(2) == 3 + C && state.size(0) == S && state.size(1) == N && ffeats.size(0) == S && ffeats.size(1) == N
                && gamma.numel() == C && beta.numel() == C && w_u.numel() == C * C && b_u.numel() == C, op, "shapes disagree");
    TORCH_CHECK(total.has_value() == dyn_mask.has_value(), op, "total and dyn_mask come together (the static pass)");
    const float *tot = nullptr, *dm = nullptr;
    if (total.has_value()) {
        tot = f32(*total, "total"); dm = f32(*dyn_mask, "dyn_mask");
        TORCH_CHECK(total->is_contiguous() && total->sizes() == state.sizes() && dyn_mask->is_contiguous() && dyn_mask->numel() == N
                    && total->device() == delta.device() && dyn_mask->device() == delta.device(), op, "total [S, N, 3], dyn_mask [N]");
    }
    at::Tensor out = at::empty_like(state);
    if (N == 0) return out;
    const int rc = bt_track_apply(delta.data_ptr<float>(), gamma.data_ptr<float>(), beta.data_ptr<float>(), w_u.data_ptr<float>(),
                                  b_u.data_ptr<float>(), state.data_ptr<float>(), ffeats.data_ptr<float>(), tot, dm, S, N, C, (float)stride,
                                  (float)dz, (float)d_range, (float)d_near, use_log_depth ? 1 : 0, out.data_ptr<float>(),
                                  c10::hip::getCurrentHIPStream(delta.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_track_apply failed with status ", rc);
    return out;
}

at::Tensor attention(const at::Tensor &qkv, int64_t heads, int64_t n_seq, int64_t L, int64_t seq_stride, int64_t tok_stride, double scale) {
    const char *op = "batrack_hip::attention: ";
    const float *p = f32(qkv, "qkv");
    TORCH_CHECK(heads >= 1 && heads <= (1 << 20) && n_seq >= 0 && L >= 1 && seq_stride >= 1 && tok_stride >= 1, op,
                "heads, L and the strides must be positive, n_seq not negative");
    const int64_t C = heads * BT_ATTN_HEAD_DIM, rows = qkv.dim() == 2 ? qkv.size(0) : 0;
    TORCH_CHECK(qkv.dim() == 2 && qkv.size(1) >= 3 * C && (qkv.size(1) == 1 || qkv.stride(1) == 1) && (rows <= 1 || qkv.stride(0) >= 3 * C),
                op, "qkv must be [rows, >= 3 * heads * ", BT_ATTN_HEAD_DIM, "] with unit last stride");
    TORCH_CHECK(n_seq <= BT_ATTN_MAX_INDEX && L <= BT_ATTN_MAX_INDEX && seq_stride <= BT_ATTN_MAX_INDEX && tok_stride <= BT_ATTN_MAX_INDEX
                && (n_seq == 0 || (n_seq - 1) * seq_stride + (L - 1) * tok_stride < rows), op, "a token addresses a row past the end of qkv");
    at::Tensor out = at::empty({rows, C}, qkv.options());
    if (n_seq == 0 || rows == 0) return out;
    const int rc = bt_attention(p, rows > 1 ? qkv.stride(0) : qkv.size(1), out.data_ptr<float>(), C, n_seq, L, seq_stride, tok_stride, heads,
                                BT_ATTN_HEAD_DIM, (float)scale, c10::hip::getCurrentHIPStream(qkv.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_attention failed with status ", rc);
    return out;
}

void rows_linear(const at::Tensor &x, const at::Tensor &w_hi, const at::Tensor &w_lo, double inv_scale, const c10::optional<at::Tensor> &bias,
                 double norm_eps, bool gelu, const c10::optional<at::Tensor> &residual, at::Tensor out, int64_t precision) {
    const char *op = "batrack_hip::rows_linear: ";
    const float *px = f32(x, "x");
    float *po = const_cast<float *>(f32(out, "out"));
    auto rows_of = [&](const at::Tensor &t, int64_t cols, const char *what) {          // [rows, cols] with unit last stride -> row stride
        TORCH_CHECK(t.dim() == 2 && t.size(0) == x.size(0) && t.size(1) == cols && (cols == 1 || t.stride(1) == 1)
                    && (t.size(0) <= 1 || t.stride(0) >= cols) && t.device() == x.device(), op, "`", what, "` must be [rows, ", cols,
                    "] with unit last stride, on the device of x");
        return t.size(0) > 1 ? t.stride(0) : cols;
    };
    TORCH_CHECK(x.dim() == 2, op, "x must be [rows, K]");
    const int64_t rows = x.size(0), K = x.size(1);
    TORCH_CHECK(w_hi.is_cuda() && w_lo.is_cuda() && w_hi.scalar_type() == at::kHalf && w_lo.scalar_type() == at::kHalf && w_hi.dim() == 2
                && w_hi.size(1) == K && w_lo.sizes() == w_hi.sizes() && w_hi.is_contiguous() && w_lo.is_contiguous()
                && w_hi.device() == x.device() && w_lo.device() == x.device(), op,
                "w_hi and w_lo must be [Nout, K] float16, contiguous, on the device of x (update_former.pack_linear)");
    const int64_t Nout = w_hi.size(0);
    TORCH_CHECK(K >= 8 && K % 8 == 0 && Nout >= 1, op, "K must be a multiple of 8 and Nout positive, got K = ", K, ", Nout = ", Nout);
    const int64_t ldx = rows_of(x, K, "x"), ldo = rows_of(out, Nout, "out");
    const float *pb = nullptr, *pr = nullptr;
    int64_t ldr = 0;
    if (bias.has_value()) {
        pb = f32(*bias, "bias");
        TORCH_CHECK(bias->dim() == 1 && bias->size(0) == Nout && bias->is_contiguous() && bias->device() == x.device(), op,
                    "bias must be [Nout], contiguous, on the device of x");
    }
    if (residual.has_value()) {
        pr = f32(*residual, "residual");
        ldr = rows_of(*residual, Nout, "residual");
    }
    TORCH_CHECK(precision == BT_ROWS_F16X3 || precision == BT_ROWS_F16, op, "precision must be BT_ROWS_F16X3 or BT_ROWS_F16");
    if (rows == 0) return;
    const int rc = bt_rows_linear(px, ldx, w_hi.data_ptr(), w_lo.data_ptr(), (float)inv_scale, pb, pr, ldr, po, ldo, rows, K, Nout,
                                  norm_eps >= 0 ? BT_ROWS_PRO_LAYERNORM : BT_ROWS_PRO_NONE, norm_eps >= 0 ? (float)norm_eps : 0.f,
                                  gelu ? BT_ROWS_ACT_GELU_TANH : BT_ROWS_ACT_NONE, (int)precision,
                                  c10::hip::getCurrentHIPStream(x.device().index()).stream());
    TORCH_CHECK(rc != BT_EINVAL, op, "bt_rows_linear refused its arguments (out must not overlap x, nor residual unless it is residual)");
    TORCH_CHECK(rc == BT_OK, op, "bt_rows_linear failed with status ", rc);
}

at::Tensor window_workspace(const at::Tensor &like) {          // zeroed: the ticket in its last word must be
    return at::zeros({(int64_t)((bt_window_workspace_bytes() + 3) / 4)}, like.options().dtype(at::kInt));
}

at::Tensor depth_range(const at::Tensor &depth, bool use_log_depth) {
    const char *op = "batrack_hip::depth_range: ";
    const float *d = f32(depth, "depth");
    TORCH_CHECK(depth.dim() == 3 && depth.numel() > 0, op, "depth must be [T, H, W] and not empty");
    at::Tensor out = at::empty({2}, depth.options()), ws = window_workspace(depth);
    const int rc = bt_depth_range(d, depth.size(0), depth.size(1), depth.size(2), depth.stride(0), depth.stride(1), depth.stride(2),
                                  use_log_depth ? 1 : 0, ws.data_ptr(), out.data_ptr<float>(),
                                  c10::hip::getCurrentHIPStream(depth.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_depth_range failed with status ", rc);
    return out;
}

std::tuple<at::Tensor, at::Tensor> window_depth(const at::Tensor &depth, int64_t S, int64_t stride, double d_near, double d_range,
                                                double dz, bool use_log_depth) {
    const char *op = "batrack_hip::window_depth: ";
    const float *d = f32(depth, "depth");
    TORCH_CHECK(depth.dim() == 3 && depth.numel() > 0 && stride >= 1 && S >= depth.size(0), op,
                "depth must be [frames <= S, H, W] and not empty, stride positive");
    at::Tensor dmaps = at::empty({S, depth.size(1) / stride, depth.size(2) / stride}, depth.options());
    at::Tensor zrange = at::empty({2}, depth.options()), ws = window_workspace(depth);
    const int rc = bt_window_depth(d, depth.size(0), S, depth.size(1), depth.size(2), depth.stride(0), depth.stride(1), depth.stride(2),
                                   stride, (float)d_near, (float)d_range, (float)dz, use_log_depth ? 1 : 0, ws.data_ptr(),
                                   dmaps.data_ptr<float>(), zrange.data_ptr<float>(),
                                   c10::hip::getCurrentHIPStream(depth.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_window_depth failed with status ", rc);
    return std::make_tuple(dmaps, zrange);
}

void embed_conv(const at::Tensor &fnet_maps, const at::Tensor &dmaps, const at::Tensor &zrange, const at::Tensor &wpacked,
                const at::Tensor &bias, const at::Tensor &freqs, int64_t frame0, at::Tensor out) {
    const char *op = "batrack_hip::embed_conv: ";
    all_f32(op, {&fnet_maps, &dmaps, &zrange, &wpacked, &bias, &freqs, &out});
    TORCH_CHECK(fnet_maps.dim() == 4 && dmaps.dim() == 3 && dmaps.is_contiguous(), op, "fnet_maps [F, C, h, w], dmaps [S, h, w] contiguous");
    const int64_t F = fnet_maps.size(0), C = fnet_maps.size(1), h = fnet_maps.size(2), w = fnet_maps.size(3), S = dmaps.size(0);
    TORCH_CHECK(C == BT_WINDOW_C, op, "the encoder's maps must have ", BT_WINDOW_C, " channels");
    TORCH_CHECK(h >= 2 && w >= 2, op, "maps of fewer than 2 rows or columns have no x or y range to normalise by");
    TORCH_CHECK(dmaps.size(1) == h && dmaps.size(2) == w && frame0 >= 0 && frame0 + F <= S, op, "dmaps must be [S, h, w] with frame0 + F <= S");
    TORCH_CHECK(zrange.numel() == 2 && zrange.is_contiguous() && bias.numel() == BT_WINDOW_C && bias.is_contiguous()
                && freqs.numel() == BT_WINDOW_FREQS && freqs.is_contiguous() && wpacked.is_contiguous()
                && wpacked.numel() == 9 * (BT_WINDOW_C + BT_WINDOW_EMB + 1) * BT_WINDOW_C, op,
                "zrange [2], bias [128], freqs [10], wpacked [24, 9, 8, 128], all contiguous");
    TORCH_CHECK(out.is_contiguous() && out.dim() == 4 && out.size(0) == F && out.size(1) == C && out.size(2) == h && out.size(3) == w, op,
                "out must be a contiguous [F, 128, h, w]");
    if (F == 0) return;
    const int rc = bt_embed_conv(fnet_maps.data_ptr<float>(), fnet_maps.stride(0), fnet_maps.stride(1), fnet_maps.stride(2), fnet_maps.stride(3),
                                 dmaps.data_ptr<float>(), zrange.data_ptr<float>(), wpacked.data_ptr<float>(), bias.data_ptr<float>(),
                                 freqs.data_ptr<float>(), S, frame0, F, h, w, C, out.data_ptr<float>(),
                                 c10::hip::getCurrentHIPStream(fnet_maps.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_embed_conv failed with status ", rc);
}

at::Tensor feat_sample(const at::Tensor &fmaps, const at::Tensor &frames, const at::Tensor &xy) {
    const char *op = "batrack_hip::feat_sample: ";
    const float *fm = f32(fmaps, "fmaps"), *pxy = f32(xy, "xy");
    TORCH_CHECK(frames.is_cuda() && frames.scalar_type() == at::kInt && frames.dim() == 1 && frames.is_contiguous(), op,
                "frames must be a contiguous int32 [n] on the GPU");
    TORCH_CHECK(fmaps.dim() == 4 && fmaps.is_contiguous() && fmaps.size(1) == BT_WINDOW_C && fmaps.numel() > 0, op,
                "fmaps must be a contiguous [S, 128, h, w]");
    const int64_t n = frames.size(0);
    TORCH_CHECK(xy.dim() == 2 && xy.size(0) == n && xy.size(1) >= 2 && (n <= 1 || xy.stride(0) >= 2) && xy.stride(1) == 1, op,
                "xy must be [n, >= 2] with unit last stride");
    TORCH_CHECK(frames.device() == fmaps.device() && xy.device() == fmaps.device(), op, "tensors must be on one device");
    at::Tensor out = at::empty({n, (int64_t)BT_WINDOW_C}, fmaps.options());
    if (n == 0) return out;
    const int rc = bt_feat_sample(fm, fmaps.size(0), fmaps.size(1), fmaps.size(2), fmaps.size(3), frames.data_ptr<int32_t>(), pxy,
                                  n > 1 ? xy.stride(0) : 2, n, out.data_ptr<float>(),
                                  c10::hip::getCurrentHIPStream(fmaps.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_feat_sample failed with status ", rc);
    return out;
}

void encoder_head(const at::Tensor &a, const at::Tensor &b, const at::Tensor &c, const at::Tensor &d, const at::Tensor &w2_packed,
                  const at::Tensor &bias2, const at::Tensor &w3_packed, const at::Tensor &bias3, at::Tensor out) {
    const char *op = "batrack_hip::encoder_head: ";
    all_f32(op, {&a, &b, &c, &d, &w2_packed, &bias2, &w3_packed, &bias3, &out});
    TORCH_CHECK(out.dim() == 4 && out.is_contiguous() && out.size(1) == BT_ENC_COUT && out.numel() > 0, op,
                "out must be a contiguous [F, 128, h, w] and not empty");
    const int64_t F = out.size(0), h = out.size(2), w = out.size(3);
    const at::Tensor *lv[4] = {&a, &b, &c, &d};
    const int64_t ch[4] = {BT_ENC_CA, BT_ENC_CB, BT_ENC_CC, BT_ENC_CD};
    bt_encoder_level L[4];
    for (int i = 0; i < 4; ++i) {
        const at::Tensor &t = *lv[i];
        TORCH_CHECK(t.dim() == 4 && t.size(0) == F && t.size(1) == ch[i] && t.size(2) >= 1 && t.size(3) >= 1, op,
                    "the levels must be [F, 64 / 96 / 128 / 128, h_l, w_l] with out's F");
        L[i] = level_of(t);
    }
    TORCH_CHECK(w2_packed.is_contiguous() && w2_packed.numel() == (int64_t)9 * BT_ENC_CIN * BT_ENC_CMID && bias2.is_contiguous()
                && bias2.numel() == BT_ENC_CMID && w3_packed.is_contiguous() && w3_packed.numel() == (int64_t)BT_ENC_CMID * BT_ENC_COUT
                && bias3.is_contiguous() && bias3.numel() == BT_ENC_COUT, op,
                "w2_packed [52, 9, 8, 256], bias2 [256], w3_packed [256, 128], bias3 [128], all contiguous");
    const size_t bytes = bt_encoder_head_workspace_bytes(F, h, w);
    TORCH_CHECK(bytes > 0, op, "F * 256 * h * w must not pass 2^31 - 1");
    at::Tensor ws = scratch(bytes, a);
    const int rc = bt_encoder_head(&L[0], &L[1], &L[2], &L[3], w2_packed.data_ptr<float>(), bias2.data_ptr<float>(), BT_ENC_CMID,
                                   w3_packed.data_ptr<float>(), bias3.data_ptr<float>(), BT_ENC_COUT, F, h, w, ws.data_ptr(),
                                   out.data_ptr<float>(), c10::hip::getCurrentHIPStream(a.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_encoder_head failed with status ", rc);
}

void res_block(const at::Tensor &x, const at::Tensor &w1, const at::Tensor &b1, const at::Tensor &w2, const at::Tensor &b2,
               const c10::optional<at::Tensor> &wd, const c10::optional<at::Tensor> &bd, int64_t stride, at::Tensor out) {
    const char *op = "batrack_hip::res_block: ";
    const bool down = wd.has_value() && wd->defined();
    TORCH_CHECK(down == (bd.has_value() && bd->defined()), op, "wd and bd come together");
    std::vector<const at::Tensor *> all = {&x, &w1, &b1, &w2, &b2, &out};
    if (down) { all.push_back(&*wd); all.push_back(&*bd); }
    all_f32(op, all);
    TORCH_CHECK(stride == 1 || stride == 2, op, "stride must be 1 or 2");
    TORCH_CHECK(down == (stride == 2), op, "wd and bd are given exactly when stride is 2");
    TORCH_CHECK(x.dim() == 4 && x.numel() > 0 && out.dim() == 4 && out.is_contiguous(), op, "x must be [F, c_in, h, w] and not empty, out contiguous");
    const int64_t F = x.size(0), c_in = x.size(1), h = x.size(2), w = x.size(3), c_out = out.size(1);
    TORCH_CHECK(out.size(0) == F && out.size(2) == (h - 1) / stride + 1 && out.size(3) == (w - 1) / stride + 1, op,
                "out must be [F, c_out, (h - 1) / stride + 1, (w - 1) / stride + 1]");
    TORCH_CHECK(w1.is_contiguous() && w1.numel() == 9 * c_in * c_out && b1.is_contiguous() && b1.numel() == c_out && w2.is_contiguous()
                && w2.numel() == 9 * c_out * c_out && b2.is_contiguous() && b2.numel() == c_out, op,
                "w1 [c_in / 8, 9, 8, c_out], b1 [c_out], w2 [c_out / 8, 9, 8, c_out], b2 [c_out], all contiguous");
    if (down) TORCH_CHECK(wd->is_contiguous() && wd->numel() == c_in * c_out && bd->is_contiguous() && bd->numel() == c_out, op,
                          "wd [c_in, c_out] and bd [c_out], contiguous");
    const size_t bytes = bt_res_block_workspace_bytes(F, c_out, h, w, stride);
    TORCH_CHECK(bytes > 0, op, "channels must be 64, 96 or 128 and the element counts must not pass 2^31 - 1");
    at::Tensor ws = scratch(bytes, x);
    const bt_encoder_level lx = level_of(x);
    const struct bt_res_block blk{w1.data_ptr<float>(), b1.data_ptr<float>(), w2.data_ptr<float>(), b2.data_ptr<float>(),
                           down ? wd->data_ptr<float>() : nullptr, down ? bd->data_ptr<float>() : nullptr, c_in, c_out, stride};
    const int rc = bt_res_block(&lx, &blk, F, ws.data_ptr(), out.data_ptr<float>(), c10::hip::getCurrentHIPStream(x.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_res_block failed with status ", rc);
}

void encoder_stem(const at::Tensor &x, const at::Tensor &w, const at::Tensor &b, at::Tensor out) {
    const char *op = "batrack_hip::encoder_stem: ";
    all_f32(op, {&x, &w, &b, &out});
    TORCH_CHECK(x.dim() == 4 && x.size(1) == BT_ENC_CIMG && x.numel() > 0 && out.dim() == 4 && out.is_contiguous(), op,
                "x must be [F, 3, h, w] and not empty, out contiguous");
    const int64_t F = x.size(0), h = x.size(2), wd = x.size(3);
    TORCH_CHECK(out.size(0) == F && out.size(1) == BT_ENC_CSTEM && out.size(2) == (h - 1) / 2 + 1 && out.size(3) == (wd - 1) / 2 + 1, op,
                "out must be [F, 64, (h - 1) / 2 + 1, (w - 1) / 2 + 1]");
    TORCH_CHECK(w.is_contiguous() && w.numel() == (int64_t)7 * BT_ENC_CIMG * 8 * BT_ENC_CSTEM && b.is_contiguous() && b.numel() == BT_ENC_CSTEM, op,
                "w [7, 3, 8, 64] and b [64], contiguous");
    const size_t bytes = bt_encoder_stem_workspace_bytes(F, h, wd);
    TORCH_CHECK(bytes > 0, op, "F * 64 * ho * wo must not pass 2^31 - 1");
    at::Tensor ws = scratch(bytes, x);
    const bt_encoder_level lx = level_of(x);
    const int rc = bt_encoder_stem(&lx, w.data_ptr<float>(), b.data_ptr<float>(), BT_ENC_CSTEM, F, ws.data_ptr(), out.data_ptr<float>(),
                                   c10::hip::getCurrentHIPStream(x.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_encoder_stem failed with status ", rc);
}

void frame_prep(const at::Tensor &image, const at::Tensor &depth, bool normalise, bool use_log_depth, at::Tensor workspace, at::Tensor rgbd,
                at::Tensor drange) {
    const char *op = "batrack_hip::frame_prep: ";
    all_f32(op, {&depth, &rgbd, &drange});
    TORCH_CHECK(image.is_cuda() && image.device() == depth.device() && (image.scalar_type() == at::kByte || image.scalar_type() == at::kFloat),
                op, "image must be uint8 or float32 on the GPU of the depth (no CPU fallback)");
    TORCH_CHECK(image.dim() == 4 && image.size(1) == 3 && depth.dim() == 3 && depth.size(0) == image.size(0) && depth.size(1) == image.size(2)
                && depth.size(2) == image.size(3) && image.size(2) >= 1 && image.size(3) >= 1, op,
                "image must be [F, 3, H, W] and depth [F, H, W], H and W at least 1");
    const int64_t F = image.size(0), H = image.size(2), W = image.size(3);
    TORCH_CHECK(rgbd.dim() == 4 && rgbd.is_contiguous() && rgbd.size(0) == F && rgbd.size(1) == 4 && rgbd.size(2) >= 1 && rgbd.size(3) >= 1
                && drange.dim() == 2 && drange.is_contiguous() && drange.size(0) == F && drange.size(1) == 2, op,
                "rgbd must be a contiguous [F, 4, oh, ow] and drange a contiguous [F, 2]");
    if (F == 0) return;
    const int64_t oh = rgbd.size(2), ow = rgbd.size(3);
    const size_t bytes = bt_frame_prep_workspace_bytes(F, oh, ow);
    TORCH_CHECK(bytes > 0, op, "F * 4 * oh * ow must not pass 2^31 - 1");
    TORCH_CHECK(workspace.is_cuda() && workspace.device() == depth.device() && workspace.scalar_type() == at::kInt && workspace.is_contiguous()
                && (size_t)workspace.numel() * 4 >= bytes, op, "workspace must be a contiguous int32 tensor of at least ", bytes, " bytes on the GPU of the frames");
    const int rc = bt_frame_prep(image.data_ptr(), image.scalar_type() == at::kByte ? 1 : 0, image.stride(0), image.stride(1), image.stride(2),
                                 image.stride(3), depth.data_ptr<float>(), depth.stride(0), depth.stride(1), depth.stride(2), F, H, W, oh, ow,
                                 normalise ? 1 : 0, use_log_depth ? 1 : 0, workspace.data_ptr(), rgbd.data_ptr<float>(), drange.data_ptr<float>(),
                                 c10::hip::getCurrentHIPStream(depth.device().index()).stream());
    TORCH_CHECK(rc == BT_OK, op, "bt_frame_prep failed with status ", rc);
}

}  // namespace

TORCH_LIBRARY(batrack_hip, m) {
    m.def("plan_create(Tensor ii, Tensor jj, Tensor kk, int n_buf, int p_tot, int fixedp, int own_lo, int own_hi) -> int", &plan_create);
    m.def("plan_destroy(int plan) -> ()", &plan_destroy);
    m.def("plan_info(int plan) -> int[]", &plan_info);
    m.def("ba_step(int plan, Tensor ws, Tensor poses, Tensor patches, Tensor mono, int mono_stride, Tensor intrinsics, Tensor targets, "
          "int target_stride, Tensor weights, Tensor(a!) poses_out, Tensor(b!) patches_out, float[] bounds, float lmbda, float ep, "
          "float alpha, int loss, bool structure_only, int phase, Tensor? lmbda_per_track=None) -> int", &ba_step);
    m.def("ba_droid(int plan, Tensor ws, Tensor poses, Tensor patches, Tensor patches_monodisp, Tensor intrinsics, Tensor targets_2d, "
          "Tensor weights, float[] bounds, float lmbda, float ep, float alpha, int loss, bool structure_only, "
          "Tensor? lmbda_per_track=None) -> (Tensor, Tensor)", &ba_droid);
    m.def("world_tracks(Tensor poses, Tensor patches, Tensor intrinsics, Tensor ix, Tensor(a!) patches_local, Tensor local_weights, "
          "int m, Tensor(b!)? points=None, Tensor(c!)? world=None) -> ()", &world_tracks);
    m.def("observe_window(Tensor traj, Tensor depth, Tensor vis, Tensor dyn, Tensor queries, Tensor? dmaps, Tensor ii, Tensor jj, Tensor kk, "
          "Tensor(a!) patches_valid, Tensor(b!) patches_local, Tensor(c!)? local_monodisp, Tensor(d!)? local_vis, Tensor(e!)? local_static, "
          "Tensor(f!)? local_weights, Tensor(g!) workspace, int n, int Sp, int kf_stride, int H, int W, float wd, float ht, int padding, "
          "float? vis_threshold, float static_quantile, float static_threshold, int min_track_len, bool is_initialized, int interp_w, "
          "int interp_h) -> (Tensor, Tensor, Tensor, Tensor)", &observe_window);
    m.def("corr_pyramid(Tensor fmaps, int levels) -> Tensor", &corr_pyramid);
    m.def("corr_lookup(Tensor pyramid, int[] shape, int levels, int radius, Tensor targets, Tensor coords) -> Tensor", &corr_lookup);
    m.def("track_pos_embed(Tensor tabx, Tensor taby, Tensor coords) -> Tensor", &track_pos_embed);
    m.def("track_tokens(Tensor coords, Tensor? coords_sub, Tensor fcorrs, Tensor ffeats, Tensor track_mask, Tensor vis, Tensor pos, "
          "Tensor time, Tensor w_flow, Tensor b_flow, bool fix_track_mask) -> Tensor", &track_tokens);
    m.def("track_apply(Tensor delta, Tensor gamma, Tensor beta, Tensor w_u, Tensor b_u, Tensor(a!) state, Tensor(b!) ffeats, "
          "Tensor? total, Tensor? dyn_mask, float stride, float dz, float d_range, float d_near, bool use_log_depth) -> Tensor", &track_apply);
    m.def("attention(Tensor qkv, int heads, int n_seq, int L, int seq_stride, int tok_stride, float scale) -> Tensor", &attention);
    m.def("rows_linear(Tensor x, Tensor w_hi, Tensor w_lo, float inv_scale, Tensor? bias, float norm_eps, bool gelu, Tensor? residual, "
          "Tensor(a!) out, int precision) -> ()", &rows_linear);
    m.def("depth_range(Tensor depth, bool use_log_depth) -> Tensor", &depth_range);
    m.def("window_depth(Tensor depth, int S, int stride, float d_near, float d_range, float dz, bool use_log_depth) -> (Tensor, Tensor)",
          &window_depth);
    m.def("embed_conv(Tensor fnet_maps, Tensor dmaps, Tensor zrange, Tensor wpacked, Tensor bias, Tensor freqs, int frame0, "
          "Tensor(a!) out) -> ()", &embed_conv);
    m.def("feat_sample(Tensor fmaps, Tensor frames, Tensor xy) -> Tensor", &feat_sample);
    m.def("encoder_head(Tensor a, Tensor b, Tensor c, Tensor d, Tensor w2_packed, Tensor bias2, Tensor w3_packed, Tensor bias3, "
          "Tensor(a!) out) -> ()", &encoder_head);
    m.def("res_block(Tensor x, Tensor w1, Tensor b1, Tensor w2, Tensor b2, Tensor? wd, Tensor? bd, int stride, Tensor(a!) out) -> ()", &res_block);
    m.def("encoder_stem(Tensor x, Tensor w, Tensor b, Tensor(a!) out) -> ()", &encoder_stem);
    m.def("frame_prep(Tensor image, Tensor depth, bool normalise, bool use_log_depth, Tensor(a!) workspace, Tensor(b!) rgbd, "
          "Tensor(c!) drange) -> ()", &frame_prep);
}
