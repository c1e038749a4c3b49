// extern "C" entry points of libvfs_hip.so (declared in include/vfs_hip.h).
#include <string.h>

#include "../../include/vfs_hip.h"
#include "../../include/vfs_hip_tuning.h"
#include "vfs_conv.h"
#include "vfs_ops.h"
#include "vfs_p2p.h"
#include "vfs_wgrad_tail.h"

static thread_local char g_err[512] = "";

int vfs_set_error(int code, const char* msg) {
  strncpy(g_err, msg, sizeof(g_err) - 1);
  g_err[sizeof(g_err) - 1] = 0;
  return code;
}
int vfs_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    char buf[400];
    snprintf(buf, sizeof(buf), "%s: launch failed: %s", what, hipGetErrorString(e));
    return vfs_set_error(VFS_ERR_LAUNCH, buf);
  }
  return VFS_OK;
}

static hipStream_t stream_of(vfs_stream_t s) { return (hipStream_t)s; }
// "<who>: <what>" as the error text: checks shared by several entry points name the one that was called
int vfs_fail(int code, const char* who, const char* what) {      // (vfs_common.h: the launchers' shared checks use it too)
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  return vfs_set_error(code, buf);
}
static int fail(int code, const char* who, const char* what) { return vfs_fail(code, who, what); }

// the A/B knobs (vfs_options.h): their definitions and the name table of vfs_set_option
#define VFS_OPTION_DEFINE(name, dflt) int vfs_option_##name = dflt;
VFS_OPTIONS(VFS_OPTION_DEFINE)
#undef VFS_OPTION_DEFINE
static const struct { const char* name; int* var; } g_options[] = {
#define VFS_OPTION_ENTRY(name, dflt) {#name, &vfs_option_##name},
    VFS_OPTIONS(VFS_OPTION_ENTRY)
#undef VFS_OPTION_ENTRY
};

static ConvGeom make_geom(int N, int H, int W, int C, int Ho, int Wo, int KH, int KW, int stride, int pad, int Ktot) {
  ConvGeom g{};
  g.N = N; g.H = H; g.W = W; g.C = C; g.Ho = Ho; g.Wo = Wo;
  g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad; g.Ktot = Ktot;
  g.M = N * Ho * Wo;
  return g;
}

// ---- one builder per argument struct: every struct is value-initialised (fields without a default are zero), an entry point
// calls the builder and then sets only what distinguishes it

// forward convolution: gather source = x [N,H,W,Cin], destination grid = y [N,Ho,Wo,Cout]
static ConvArgs conv_fwd_args(const vfs_bf16* x, const vfs_bf16* wf, vfs_bf16* y, const float* bias, float* stats, int N, int H, int W,
                              int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad) {
  ConvArgs a{};
  a.g = make_geom(N, H, W, Cin, Ho, Wo, KH, KW, stride, pad, KH * KW * Cin);
  a.src = x; a.wgt = wf; a.out = y; a.bias = bias; a.stats = stats; a.Cout = Cout;
  return a;
}
// dgrad: gather source = dy [N,Ho,Wo,Cout]; destination grid = dx [N,H,W,Cin]
static ConvArgs conv_dgrad_args(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, int N, int H, int W, int Cin,
                                int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad) {
  ConvArgs a{};
  a.g = make_geom(N, Ho, Wo, Cout, H, W, KH, KW, stride, pad, KH * KW * Cout);
  a.src = dy; a.wgt = wd; a.out = dx; a.add = add; a.Cout = Cin;
  return a;
}
// the 7x7 / stride-2 stem on NHWC4 input, and which of its two kernels takes it: the direct kernel (stem.hip), else GATHER_STEM
static ConvArgs stem_fwd_args(const vfs_bf16* x4, const vfs_bf16* wf, vfs_bf16* y, float* stats, int N, int H, int Wp, int Ho, int Wo) {
  ConvArgs a = conv_fwd_args(x4, wf, y, nullptr, stats, N, H, Wp, 4, Ho, Wo, 64, 7, 7, 2, 3);
  a.g.Ktot = 256;      // 8 x 8 x 4: the taps and channels as the stem gather pads them (vfs_conv.h, GATHER_STEM)
  return a;
}
static bool stem_takes_direct(const ConvArgs& a) { return vfs_option_stem_direct && (size_t)a.g.N * a.g.H * a.g.W * 8 < 0xFFFFFFF0ull; }
static int set_add_mask(ConvArgs& a, const vfs_bf16* add, const uint8_t* add_mask, int N, int H, int W, int Cin) {
  if (!add_mask) return VFS_OK;
  if (!add || Cin % 64) return vfs_set_error(VFS_ERR_SHAPE, "conv_dgrad: add_mask needs an add operand and Cin % 64 == 0");
  a.add_mask = add_mask; a.add_rows = (long long)N * H * W;
  return VFS_OK;
}

static WgradArgs wgrad_args(const vfs_bf16* dy, const vfs_bf16* x, const float* in_bnp, int in_npg, float* partial, int N, int H, int W,
                            int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int nsplit, int pix_per_split) {
  WgradArgs a{};
  a.g = make_geom(N, H, W, Cin, Ho, Wo, KH, KW, stride, pad, KH * KW * Cin);
  a.dy = dy; a.x = x; a.partial = partial; a.Cout = Cout; a.pix_per_split = pix_per_split; a.nsplit = nsplit;
  a.in_bnp = in_bnp; a.in_npg = in_npg;
  return a;
}
// the tail of a weight gradient whose kernel used `nsplit` splits: reduce the partials into grad now, or (grad == null) leave them to
// the caller's vfs_wgrad_reduce_table - its table needs the split count it offered, so plan_error (when given) is raised if the
// kernel took fewer.  Cin: channels of the OIHW gradient (the stem: 3 of the 4 stored ones).
static int finish_wgrad(const WgradArgs& a, float* grad, int nsplit, int Cin, int stem, const char* plan_error, hipStream_t stream) {
  if (!grad) return plan_error && nsplit != a.nsplit ? vfs_set_error(VFS_ERR_SHAPE, plan_error) : VFS_OK;
  return vfs_wgrad_reduce_launch(a.partial, grad, nsplit, a.Cout, a.g.Ktot, Cin, a.g.KH, a.g.KW, stem, stream);
}

static BnActArgs bn_act_args(const vfs_bf16* x, const float* bnp, const vfs_bf16* res, const vfs_bf16* rres, const float* rbnp, vfs_bf16* y,
                             uint8_t* mask_bits, long long M, int C, int mpg, int relu) {
  BnActArgs a{};
  a.x = x; a.bnp = bnp; a.res = res; a.rres = rres; a.rbnp = rbnp; a.y = y; a.M = M; a.C = C; a.mpg = mpg; a.relu = relu;
  a.mbits = mask_bits;
  return a;
}
// in-kernel statistics finalisation of the forward apply pass (G = M / mpg groups) ...
static BnFin bn_fin_fwd(const float* partial, int bpg, int G, const float* gamma, const float* beta, float* bnp, double* sums,
                        float* running_mean, float* running_var, double count, float eps, float momentum) {
  BnFin f{};
  f.partial = partial; f.bpg = bpg; f.G = G; f.gamma = gamma; f.beta = beta; f.bnp = bnp; f.sums = sums;
  f.running_mean = running_mean; f.running_var = running_var; f.count = count; f.eps = eps; f.momentum = momentum;
  return f;
}
// ... and of the backward one
static BnFin bn_fin_bwd(const float* partial, int bpg, int G, double* sums, float* dgamma, float* dbeta) {
  BnFin f{};
  f.partial = partial; f.bpg = bpg; f.G = G; f.sums = sums; f.dgamma = dgamma; f.dbeta = dbeta;
  return f;
}
// BatchNorm backward: the operands of both passes and the outputs of pass 2 (dx, gm, count; pass 1 has none of them); what a pass
// adds - partial / ppb, sums - is set by its entry point
static BnBwdArgs bn_bwd_args(const vfs_bf16* g, const vfs_bf16* y, const vfs_bf16* x, const float* bnp, vfs_bf16* dx, vfs_bf16* gm,
                             long long M, int C, int mpg, double count, int relu) {
  BnBwdArgs a{};
  a.g = g; a.y = y; a.x = x; a.bnp = bnp; a.dx = dx; a.gm = gm; a.M = M; a.C = C; a.mpg = mpg; a.count = count; a.relu = relu;
  return a;
}
static P2PTail make_tail(const void* peers, int rank, int world, void* state, long long spin_limit, int seq = 0) {
  P2PTail x{};
  x.peers = (void* const*)peers; x.rank = rank; x.world = world; x.state = (unsigned long long*)state;
  x.spin_limit = (unsigned long long)(spin_limit < 1 ? 1 : spin_limit);
  x.seq = seq;
  return x;
}
// preconditions of the apply passes with the SyncBN exchange folded in (vfs_bn_act_fin_xchg, vfs_bn_bwd_apply_fin_xchg)
static int xchg_check(const char* who, int seq, const void* peers, const void* state, const void* partial) {
  if (seq < 0 || seq >= 4095) return fail(VFS_ERR_ARG, who, "0 <= seq < 4095");
  if (!peers || !state || !partial) return fail(VFS_ERR_ARG, who, "statistics rows, peers and state must be given");
  return VFS_OK;
}
static StemBwdArgs stem_bwd_args(const vfs_bf16* gp, const vfs_bf16* yp, const uint8_t* idx, const vfs_bf16* x, const float* bnp, int N,
                                 int H, int W, int C, int Hp, int Wp, int npg) {
  StemBwdArgs a{};
  a.gp = gp; a.yp = yp; a.idx = idx; a.x = x; a.bnp = bnp;
  a.N = N; a.H = H; a.W = W; a.C = C; a.Hp = Hp; a.Wp = Wp; a.npg = npg;
  return a;
}
static LossArgs loss_args(const vfs_bf16* p1, const vfs_bf16* z1, const vfs_bf16* p2, const vfs_bf16* z2, int N, int C, int T, int K,
                          int negative, float weight) {
  LossArgs a{};
  a.p1 = p1; a.z1 = z1; a.p2 = p2; a.z2 = z2; a.N = N; a.C = C; a.T = T; a.K = K; a.negative = negative; a.weight = weight;
  return a;
}
// the per-position loss of DenseSimSiamHead: what forward and backward check alike, then the operands they share
static int dense_loss_check(const char* who, const vfs_bf16* p1, const vfs_bf16* z1, const vfs_bf16* p2, const vfs_bf16* z2, int N, int S,
                            int C, int T, int K) {
  if (T < 1 || N < 1 || N % T) return fail(VFS_ERR_SHAPE, who, "N % T");
  if (K < 1 || K > T) return fail(VFS_ERR_SHAPE, who, "1 <= K <= T");
  if (S < 1) return fail(VFS_ERR_SHAPE, who, "S >= 1");
  if (C < 8 || C % 8) return fail(VFS_ERR_SHAPE, who, "C % 8");
  if (C > VFS_DENSE_LOSS_MAX_C) return fail(VFS_ERR_SHAPE, who, "C > 2048");
  if (!p1 || !z1 || !p2 || !z2 || (((size_t)p1 | (size_t)z1 | (size_t)p2 | (size_t)z2) & 15)) return fail(VFS_ERR_ARG, who, "null or unaligned operand (16 bytes)");
  return VFS_OK;
}
static long long dense_loss_workspace_need(int N, int S, int C, int K) { return (long long)K * N * vfs_dense_loss_split(S, C) * 2 * 4; }
static DenseLossArgs dense_loss_args(const vfs_bf16* p1, const vfs_bf16* z1, const vfs_bf16* p2, const vfs_bf16* z2, int N, int S, int C,
                                     int T, int K, int negative, float weight) {
  DenseLossArgs a{};
  a.p1 = p1; a.z1 = z1; a.p2 = p2; a.z2 = z2; a.N = N; a.S = S; a.C = C; a.T = T; a.K = K; a.negative = negative; a.weight = weight;
  return a;
}

// label propagation: the key list, the dense kernels' workspace (dense_workspace = false: the caller has a requirement of its own)
// and the unmasked prefix of the key list (radius <= 0, no spatial mask: every key frame may be "unmasked")
static long long lp_workspace_need(int H, int W) { return (long long)LP_MAX_SPLIT * H * W * 10 * 8; }
static int lp_check(const char* who, int nkeys, int radius, int non_mask_len, bool dense_workspace, const void* workspace,
                    long long workspace_bytes, int H, int W) {
  if (nkeys < 1 || nkeys > LP_MAX_KEYS) return fail(VFS_ERR_SHAPE, who, "1 <= nkeys <= 64");
  if (dense_workspace && (H <= 0 || W <= 0 || !workspace || workspace_bytes < lp_workspace_need(H, W)))
    return fail(VFS_ERR_ARG, who, "workspace smaller than vfs_labelprop_workspace_bytes(H, W)");
  if (non_mask_len < 0 || non_mask_len >= nkeys + (radius <= 0)) return fail(VFS_ERR_ARG, who, "0 <= non_mask_len < nkeys");
  return VFS_OK;
}
static void lp_fill_kslot(int (&dst)[LP_MAX_KEYS], const int* kslot, int nkeys) {      // kslot is a HOST array
  for (int i = 0; i < LP_MAX_KEYS; ++i) dst[i] = i < nkeys ? kslot[i] : 0;
}
// the dense kernels' workspace: [LP_MAX_SPLIT][H*W][10] partial top-k values, then as many key ids
static int* lp_pidx(void* workspace, int H, int W) { return workspace ? (int*)((float*)workspace + (size_t)LP_MAX_SPLIT * H * W * 10) : nullptr; }
static LabelPropF32Args lp_f32_args(const float* fbank, const float* sbank, float* out, void* workspace, int qframe, const int* kslot,
                                    int nkeys, int H, int W, int C, int CO, int radius, int non_mask_len, int topk, float temperature) {
  LabelPropF32Args a{};
  a.fbank = fbank; a.sbank = sbank; a.out = out; a.qframe = qframe; a.nkeys = nkeys;
  a.pval = (float*)workspace; a.pidx = lp_pidx(workspace, H, W);
  lp_fill_kslot(a.kslot, kslot, nkeys);
  a.H = H; a.W = W; a.C = C; a.CO = CO; a.radius = radius; a.topk = topk; a.temperature = temperature; a.non_mask_len = non_mask_len;
  return a;
}

static PipelineArgs pipeline_args(const uint8_t* src, const int* boxes, const uint8_t* flips, float* imgs, vfs_bf16* x4, int B, int V, int T,
                                  int Hs, int Ws, int Ho, int Wo, int Wp, double mean_r, double mean_g, double mean_b, double std_r,
                                  double std_g, double std_b) {
  PipelineArgs a{};
  a.src = src; a.boxes = boxes; a.flips = flips; a.imgs = imgs; a.x4 = x4;
  a.B = B; a.V = V; a.T = T; a.Hs = Hs; a.Ws = Ws; a.Ho = Ho; a.Wo = Wo; a.Wp = Wp;
  a.mean[0] = mean_r; a.mean[1] = mean_g; a.mean[2] = mean_b;
  a.stdinv[0] = 1.0 / std_r; a.stdinv[1] = 1.0 / std_g; a.stdinv[2] = 1.0 / std_b;
  return a;
}

// the ragged entries describe the source per sample instead of by one Hs, Ws pair (which they leave 0)
static PipelineArgs ragged_args(PipelineArgs a, const int* srcdesc, long long src_bytes) {
  a.srcdesc = srcdesc; a.src_bytes = src_bytes; a.ragged = true;
  return a;
}

// the argument checks of the uniform and the ragged pipeline entries (an empty source buffer is refused like a null one)
static int pipeline_check(const char* who, const PipelineArgs& a, const void* photo) {
  if (!a.src || !a.boxes || !a.flips || !photo || (!a.imgs && !a.x4) || (a.ragged && (!a.srcdesc || a.src_bytes <= 0)))
    return fail(VFS_ERR_ARG, who, "null buffer");
  if (a.x4 && a.Wp < a.Wo) return fail(VFS_ERR_SHAPE, who, "Wp < Wo");
  return VFS_OK;
}

static int pipeline_run(const char* who, const PipelineArgs& a, hipStream_t s) {
  const int rc = pipeline_check(who, a, a.src);
  return rc != VFS_OK ? rc : vfs_crop_resize_flip_norm_launch(a, s);
}

// max_blur_radius: 0 for the entry points whose rows carry no radius, 0..3 from the _blur ones
static int photo_run(const char* who, const PipelineArgs& a, const int* photo, void* workspace, long long workspace_bytes, int max_blur_radius,
                     hipStream_t s) {
  const int rc = pipeline_check(who, a, photo);
  if (rc != VFS_OK) return rc;
  if (max_blur_radius < 0 || max_blur_radius > 3) return fail(VFS_ERR_SHAPE, who, "max_blur_radius outside 0..3");
  if (a.B <= 0 || a.V <= 0 || a.T <= 0 || a.Ho <= 0 || a.Wo <= 0) return fail(VFS_ERR_SHAPE, who, "empty batch");
  if (!workspace || workspace_bytes < vfs_photo_workspace_bytes(a.B * a.V * a.T, a.Ho, a.Wo))
    return fail(VFS_ERR_ARG, who, "workspace smaller than vfs_crop_resize_flip_photo_norm_workspace_bytes");
  PhotoArgs pa{};
  pa.p = a;
  pa.photo = photo;
  pa.sums = (unsigned long long*)workspace;
  pa.pix = (uint32_t*)((char*)workspace + (size_t)a.B * a.V * a.T * 8);
  pa.max_blur_radius = max_blur_radius;
  return vfs_crop_resize_flip_photo_norm_launch(pa, s);
}

extern "C" {

const char* vfs_last_error(void) { return g_err; }
int vfs_abi_version(void) { return 3; }      // 2: vfs_sgd_step(skip_flag), vfs_labelprop*(workspace_bytes); 3: batched post-processing (Tmaps), desc [5]
int vfs_set_option(const char* name, int value) {
  for (const auto& o : g_options) {
    if (strcmp(name, o.name)) continue;
    if (o.var == &vfs_option_bn_chunk_rows) value = value > 0 ? value : 64;
    if (o.var == &vfs_option_lp2_cap) value = value <= 0 ? 0 : (value < 16 ? 16 : value);
    *o.var = value;
    return VFS_OK;
  }
  return vfs_set_error(VFS_ERR_ARG, "vfs_set_option: unknown option");
}

int vfs_imgs_to_nhwc4(const float* imgs, vfs_bf16* out, int B, int V, int T, int H, int W, int Wp, vfs_stream_t stream) {
  if (Wp < W || (Wp & 1)) return vfs_set_error(VFS_ERR_SHAPE, "imgs_to_nhwc4: Wp must be even and >= W");
  return vfs_imgs_to_nhwc4_launch(imgs, out, B, V, T, H, W, Wp, stream_of(stream));
}

int vfs_pack_weights(const void* desc, int ntensors, long long total, vfs_stream_t stream) {
  return vfs_pack_weights_launch((const PackDesc*)desc, ntensors, total, stream_of(stream));
}

int vfs_conv_fwd(const vfs_bf16* x, const vfs_bf16* wf, vfs_bf16* y, const float* bias, float* stats, int N, int H, int W,
                 int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, vfs_stream_t stream) {
  const ConvArgs a = conv_fwd_args(x, wf, y, bias, stats, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad);
  return vfs_conv_igemm_dispatch(a, GATHER_FWD, stream_of(stream));
}
int vfs_conv_fwd_coarse(const vfs_bf16* x, const vfs_bf16* wf, vfs_bf16* y, const float* bias, float* stats, float* stats_coarse,
                        uint32_t* tickets, int coarse_log2, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW,
                        int stride, int pad, vfs_stream_t stream) {
  if (!stats || !stats_coarse || !tickets || coarse_log2 < 1 || coarse_log2 > 8)
    return vfs_set_error(VFS_ERR_ARG, "conv_fwd_coarse: stats, stats_coarse, tickets and 1 <= coarse_log2 <= 8");
  ConvArgs a = conv_fwd_args(x, wf, y, bias, stats, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad);
  a.stats_coarse = stats_coarse; a.stats_tickets = tickets; a.coarse_log2 = coarse_log2;
  return vfs_conv_igemm_dispatch(a, GATHER_FWD, stream_of(stream));
}
int vfs_conv_fwd_dilated(const vfs_bf16* x, const vfs_bf16* wf, vfs_bf16* y, const float* bias, float* stats, int N, int H, int W,
                         int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int dilation, vfs_stream_t stream) {
  if (dilation < 1) return vfs_set_error(VFS_ERR_ARG, "conv_fwd_dilated: dilation >= 1");
  if (Ho != (H + 2 * pad - dilation * (KH - 1) - 1) / stride + 1 || Wo != (W + 2 * pad - dilation * (KW - 1) - 1) / stride + 1)
    return vfs_set_error(VFS_ERR_SHAPE, "conv_fwd_dilated: output size does not match (H + 2 pad - dilation (K - 1) - 1) / stride + 1");
  ConvArgs a = conv_fwd_args(x, wf, y, bias, stats, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad);
  a.g.dil = dilation;
  return vfs_conv_igemm_dispatch(a, GATHER_FWD, stream_of(stream));
}
int vfs_conv_fwd_splitk(const vfs_bf16* x, const vfs_bf16* wf, vfs_bf16* y, const float* bias, float* stats, float* ks_ws, int ksplit,
                        int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                        vfs_stream_t stream) {
  if (ksplit < 1 || (ksplit > 1 && !ks_ws)) return vfs_set_error(VFS_ERR_ARG, "conv_fwd_splitk: workspace");
  ConvArgs a = conv_fwd_args(x, wf, y, bias, stats, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad);
  a.ks_ws = ks_ws; a.ksplit = ksplit;
  return vfs_conv_igemm_dispatch(a, GATHER_FWD, stream_of(stream));
}
int vfs_conv_dgrad_splitk(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, float* ks_ws, int ksplit, int N,
                          int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                          vfs_stream_t stream) {
  if (ksplit < 1 || (ksplit > 1 && !ks_ws)) return vfs_set_error(VFS_ERR_ARG, "conv_dgrad_splitk: workspace");
  if (stride != 1) return vfs_set_error(VFS_ERR_SHAPE, "conv_dgrad_splitk: stride 1 only");
  ConvArgs a = conv_dgrad_args(dy, wd, dx, add, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad);
  a.ks_ws = ks_ws; a.ksplit = ksplit;
  return vfs_conv_igemm_dispatch(a, GATHER_DGRAD, stream_of(stream));
}
int vfs_conv_fwd_bnin(const vfs_bf16* x_raw, const float* in_bnp, int in_npg, const vfs_bf16* wf, vfs_bf16* y, const float* bias,
                      float* stats, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                      vfs_stream_t stream) {
  if (!in_bnp || in_npg <= 0) return vfs_set_error(VFS_ERR_ARG, "conv_fwd_bnin: BatchNorm parameters of the input");
  ConvArgs a = conv_fwd_args(x_raw, wf, y, bias, stats, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad);
  a.in_bnp = in_bnp; a.in_npg = in_npg;
  const bool smallw = vfs_small_map(H, W);
  // round 6: also the 1x1 / stride-1 forward of the implicit-GEMM kernel (the conv2 -> conv3 edge), groups of whole 128-pixel tiles
  const bool pw = KH * KW == 1 && stride == 1 && pad == 0 && H == Ho && W == Wo && Cin % 64 == 0 && ((long long)in_npg * H * W) % 128 == 0;
  if (pw) return vfs_conv_igemm_dispatch(a, GATHER_FWD, stream_of(stream));
  if (!vfs_takes_halo(a, GATHER_FWD) || (smallw && in_npg % 2))
    return vfs_set_error(VFS_ERR_SHAPE, "conv_fwd_bnin: the 3x3/stride-1 halo-tile kernel and the 1x1/stride-1 kernel fold the input BatchNorm");
  return vfs_conv_igemm_dispatch(a, GATHER_FWD, stream_of(stream));
}

int vfs_stem_fwd(const vfs_bf16* x4, const vfs_bf16* wf, vfs_bf16* y, float* stats, int N, int H, int Wp, int Ho, int Wo,
                 vfs_stream_t stream) {
  if (Wp & 1) return vfs_set_error(VFS_ERR_SHAPE, "stem_fwd: padded width must be even");
  const ConvArgs a = stem_fwd_args(x4, wf, y, stats, N, H, Wp, Ho, Wo);
  if (stem_takes_direct(a)) return vfs_stem_fwd_direct_launch(a, stream_of(stream));
  return vfs_conv_igemm_dispatch(a, GATHER_STEM, stream_of(stream));
}

int vfs_conv_dgrad_maskadd(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, const uint8_t* add_mask, int N,
                           int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, vfs_stream_t stream) {
  // the downsample branch of a stage entry: a 1x1 / stride-2 / pad-0 dgrad that completes the residual branch's gradient IN PLACE.
  // Three of its four parity classes have no tap - their workgroups would copy `add` to itself - so only the quarter grid runs
  // (vfs_conv_dgrad_ds); every pixel of dx ends with the value the four classes would leave.
  if (vfs_option_igemm_ds_quarter && KH == 1 && KW == 1 && stride == 2 && pad == 0 && add && add == dx && !add_mask && H >= 1 && W >= 1 &&
      Ho == (H + 1) / 2 && Wo == (W + 1) / 2)
    return vfs_conv_dgrad_ds(dy, wd, dx, add, 0, N, H, W, Cin, Ho, Wo, Cout, stream);
  ConvArgs a = conv_dgrad_args(dy, wd, dx, add, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad);
  if (int rc = set_add_mask(a, add, add_mask, N, H, W, Cin)) return rc;
  return vfs_conv_igemm_dispatch(a, GATHER_DGRAD, stream_of(stream));
}
int vfs_conv_dgrad(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, int N, int H, int W, int Cin,
                   int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, vfs_stream_t stream) {
  return vfs_conv_dgrad_maskadd(dy, wd, dx, add, nullptr, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, stream);
}
// dgrad of a 1x1 / stride-2 / pad-0 convolution on the quarter grid: a 1x1 / stride-1 dgrad over the Ho x Wo pixels of dy, whose
// output rows are the compact tensor's (compact) or the even-even pixels of the dense one (a.out_H, a.out_W: GATHER_DGRADQ)
static int conv_dgrad_ds_args(ConvArgs& a, const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, int compact, int N,
                              int H, int W, int Cin, int Ho, int Wo, int Cout) {
  if (N < 1 || H < 1 || W < 1 || Ho != (H + 1) / 2 || Wo != (W + 1) / 2)
    return vfs_set_error(VFS_ERR_SHAPE, "conv_dgrad_ds: Ho = ceil(H / 2), Wo = ceil(W / 2) of a 1x1 / stride-2 / pad-0 convolution");
  a = conv_dgrad_args(dy, wd, dx, add, N, Ho, Wo, Cin, Ho, Wo, Cout, 1, 1, 1, 0);
  if (!compact) { a.out_H = H; a.out_W = W; }
  return VFS_OK;
}
int vfs_conv_dgrad_ds(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, int compact, int N, int H, int W,
                      int Cin, int Ho, int Wo, int Cout, vfs_stream_t stream) {
  if (!dy || !wd || !dx) return vfs_set_error(VFS_ERR_ARG, "conv_dgrad_ds: null operand");
  ConvArgs a{};
  if (int rc = conv_dgrad_ds_args(a, dy, wd, dx, add, compact, N, H, W, Cin, Ho, Wo, Cout)) return rc;
  return vfs_conv_igemm_dispatch(a, GATHER_DGRAD, stream_of(stream));
}
int vfs_conv_dgrad_ds_plan(int compact, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int* wide, int* ring) {
  if (!wide || !ring) return vfs_set_error(VFS_ERR_ARG, "conv_dgrad_ds_plan: bad argument");
  ConvArgs a{};
  if (int rc = conv_dgrad_ds_args(a, nullptr, nullptr, nullptr, nullptr, compact, N, H, W, Cin, Ho, Wo, Cout)) return rc;
  const IgemmTiling tl = vfs_conv_igemm_tiling(a, GATHER_DGRAD);
  *wide = tl.wide; *ring = tl.ring;
  return VFS_OK;
}
int vfs_conv_dgrad_bn_maskadd(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, const uint8_t* add_mask,
                              const vfs_bf16* bn_x, const vfs_bf16* bn_y, const float* bnp, float* bn_partial, int bn_mpg, int bn_relu,
                              int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                              vfs_stream_t stream) {
  if (stride != 1) return vfs_set_error(VFS_ERR_SHAPE, "conv_dgrad_bn: stride 1 only (strided dgrads run per parity class)");
  if (!bn_x || !bnp || !bn_partial || bn_mpg <= 0) return vfs_set_error(VFS_ERR_ARG, "conv_dgrad_bn: null statistics operand");
  const long long M = (long long)N * H * W;
  ConvArgs a = conv_dgrad_args(dy, wd, dx, add, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad);
  if (int rc = set_add_mask(a, add, add_mask, N, H, W, Cin)) return rc;
  a.bn.x = bn_x; a.bn.y = bn_y; a.bn.bnp = bnp; a.bn.partial = bn_partial; a.bn.mpg = bn_mpg; a.bn.relu = bn_relu;
  // a statistics row must belong to ONE group: spatial tiles never straddle images (halo kernels: groups of whole
  // images), linear blocks are 128 pixels
  const bool tiles = vfs_takes_halo(a, GATHER_DGRAD);
  if (bn_mpg < M && (tiles ? bn_mpg % ((long long)H * W) != 0 : bn_mpg % 128 != 0))
    return vfs_set_error(VFS_ERR_SHAPE, "conv_dgrad_bn: groups must be whole images (tile kernels) / multiples of 128 pixels");
  return vfs_conv_igemm_dispatch(a, GATHER_DGRAD, stream_of(stream));
}
int vfs_conv_dgrad_bn(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, const vfs_bf16* bn_x,
                      const vfs_bf16* bn_y, const float* bnp, float* bn_partial, int bn_mpg, int bn_relu, int N, int H, int W,
                      int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, vfs_stream_t stream) {
  return vfs_conv_dgrad_bn_maskadd(dy, wd, dx, add, nullptr, bn_x, bn_y, bnp, bn_partial, bn_mpg, bn_relu, N, H, W, Cin, Ho, Wo, Cout,
                                   KH, KW, stride, pad, stream);
}

int vfs_conv_wgrad(const vfs_bf16* dy, const vfs_bf16* x, float* partial, float* grad, int N, int H, int W, int Cin, int Ho,
                   int Wo, int Cout, int KH, int KW, int stride, int pad, int nsplit, int pix_per_split, vfs_stream_t stream) {
  const WgradArgs a = wgrad_args(dy, x, nullptr, 0, partial, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, nsplit, pix_per_split);
  int rc;
  if (vfs_takes_halo(a)) {
    rc = vfs_wgrad_halo_dispatch(a, stream_of(stream), &nsplit);   // may use fewer splits than offered
  } else {
    rc = vfs_conv_wgrad_dispatch(a, GATHER_FWD, stream_of(stream));
  }
  if (rc) return rc;
  return finish_wgrad(a, grad, nsplit, Cin, 0, "conv_wgrad: deferred reduction needs a split plan the kernel takes as offered", stream_of(stream));
}
int vfs_conv_wgrad_bnin(const vfs_bf16* dy, const vfs_bf16* x_raw, const float* in_bnp, int in_npg, float* partial, float* grad, int N,
                        int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int nsplit,
                        int pix_per_split, vfs_stream_t stream) {
  if (!in_bnp || in_npg <= 0) return vfs_set_error(VFS_ERR_ARG, "conv_wgrad_bnin: BatchNorm parameters of the input");
  const WgradArgs a = wgrad_args(dy, x_raw, in_bnp, in_npg, partial, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, nsplit, pix_per_split);
  if (KH * KW == 1 && stride == 1 && pad == 0 && H == Ho && W == Wo) {      // round 6: the 1x1 / stride-1 kernel (register-staged) folds it too
    int rc1 = vfs_conv_wgrad_dispatch(a, GATHER_FWD, stream_of(stream));
    if (rc1) return rc1;
    return finish_wgrad(a, grad, nsplit, Cin, 0, nullptr, stream_of(stream));      // (this kernel takes every plan as offered)
  }
  if (!vfs_takes_halo(a) || (vfs_small_map(H, W) && in_npg % 2))
    return vfs_set_error(VFS_ERR_SHAPE, "conv_wgrad_bnin: the 3x3/stride-1 halo-tile kernel and the 1x1/stride-1 kernel fold the input BatchNorm");
  int rc = vfs_wgrad_halo_dispatch(a, stream_of(stream), &nsplit);
  if (rc) return rc;
  return finish_wgrad(a, grad, nsplit, Cin, 0, "conv_wgrad_bnin: deferred reduction needs a split plan the kernel takes as offered", stream_of(stream));
}

int vfs_wgrad_tickets(void) { return VFS_WGRAD_TICKETS; }
int vfs_conv_wgrad_inl(const vfs_bf16* dy, const vfs_bf16* x, const float* in_bnp, int in_npg, float* partial, float* grad,
                       unsigned* tickets, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                       int pad, int nsplit, int pix_per_split, vfs_stream_t stream) {
  if (!grad || !tickets || !partial) return vfs_set_error(VFS_ERR_ARG, "conv_wgrad_inl: partial, grad and tickets must be given");
  if (in_bnp && in_npg <= 0) return vfs_set_error(VFS_ERR_ARG, "conv_wgrad_inl: images per BatchNorm group of the input");
  WgradArgs a = wgrad_args(dy, x, in_bnp, in_bnp ? in_npg : 0, partial, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, nsplit, pix_per_split);
  a.grad = grad; a.tickets = tickets;
  if (vfs_takes_halo(a) && !(in_bnp && vfs_small_map(H, W) && in_npg % 2))
    return vfs_wgrad_halo_dispatch(a, stream_of(stream), &nsplit);
  if (in_bnp) return vfs_set_error(VFS_ERR_SHAPE, "conv_wgrad_inl: only the 3x3/stride-1 halo-tile kernel folds the input BatchNorm");
  return vfs_conv_wgrad_dispatch(a, GATHER_FWD, stream_of(stream));
}

int vfs_stem_wgrad(const vfs_bf16* dy, const vfs_bf16* x4, float* partial, float* grad, int N, int H, int Wp, int Ho, int Wo,
                   int nsplit, int pix_per_split, vfs_stream_t stream) {
  WgradArgs a = wgrad_args(dy, x4, nullptr, 0, partial, N, H, Wp, 4, Ho, Wo, 64, 7, 7, 2, 3, nsplit, pix_per_split);
  a.g.Ktot = 256;      // (as vfs_stem_fwd)
  int rc = vfs_conv_wgrad_dispatch(a, GATHER_STEM, stream_of(stream));
  if (rc) return rc;
  return finish_wgrad(a, grad, nsplit, 3, 1, nullptr, stream_of(stream));      // (this kernel takes every plan as offered)
}

// ---- the tiling plan behind the launches above (host only: nothing is launched).  Each query builds the argument struct with the
// entry point's own builder and asks the predicate its dispatcher asks.
// rows of ONE launch over all G groups, per group - or 0: a group does not own whole rows
static int rows_per_group(bool tiles, int total, int N, int G, long long pixels_per_image) {
  if (N % G) return 0;
  if (tiles) return total % G == 0 ? total / G : 0;      // (spatial tiles never straddle images; whole image PAIRS: total = N / 2)
  return G == 1 || ((N / G) * pixels_per_image) % 128 == 0 ? (total + G - 1) / G : 0;
}
int vfs_conv_plan(int dgrad, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int dilation,
                  int G, int* halo, int* rows, int* pairs) {
  if (!halo || !rows || !pairs || G < 1 || dilation < 1) return vfs_set_error(VFS_ERR_ARG, "conv_plan: bad argument");
  ConvArgs a = dgrad ? conv_dgrad_args(nullptr, nullptr, nullptr, nullptr, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad)
                     : conv_fwd_args(nullptr, nullptr, nullptr, nullptr, nullptr, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad);
  a.g.dil = dilation;
  *halo = vfs_takes_halo(a, dgrad ? GATHER_DGRAD : GATHER_FWD);
  *pairs = *halo && vfs_small_map(a.g.H, a.g.W);
  if (dgrad && stride != 1) *rows = 0;      // (strided dgrads run per parity class and write no statistics rows)
  else *rows = rows_per_group(*halo, *halo ? vfs_conv_halo_stats_rows(a) : vfs_conv_igemm_stats_rows(a), N, G, (long long)a.g.Ho * a.g.Wo);
  return VFS_OK;
}
int vfs_stem_plan(int N, int H, int Wp, int Ho, int Wo, int G, int* rows) {
  if (!rows || G < 1) return vfs_set_error(VFS_ERR_ARG, "stem_plan: bad argument");
  const ConvArgs a = stem_fwd_args(nullptr, nullptr, nullptr, nullptr, N, H, Wp, Ho, Wo);
  const bool direct = stem_takes_direct(a);
  *rows = rows_per_group(direct, direct ? vfs_stem_tiles(N, Ho, Wo) : vfs_conv_igemm_stats_rows(a), N, G, (long long)Ho * Wo);
  return VFS_OK;
}
int vfs_conv_wgrad_plan(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int* halo,
                        int* ntiles) {
  if (!halo || !ntiles) return vfs_set_error(VFS_ERR_ARG, "conv_wgrad_plan: bad argument");
  const WgradArgs a = wgrad_args(nullptr, nullptr, nullptr, 0, nullptr, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, 1, 64);
  *halo = vfs_takes_halo(a);
  *ntiles = *halo ? vfs_wgrad_halo_tiles(a) : 0;
  return VFS_OK;
}

int vfs_wgrad_reduce_table(const void* desc, int nrecords, int total_blocks, vfs_stream_t stream) {
  if (nrecords > 0 && !desc) return vfs_set_error(VFS_ERR_ARG, "wgrad_reduce_table: null table");
  return vfs_wgrad_reduce_table_launch((const WgradReduceDesc*)desc, nrecords, total_blocks, stream_of(stream));
}

int vfs_bias_grad(const vfs_bf16* dy, float* db, int M, int C, vfs_stream_t stream) {
  return vfs_bias_grad_launch(dy, db, M, C, stream_of(stream));
}

int vfs_bn_reduce_partials(const float* partial, double* sums, double* scratch, int G, int bpg, int C, vfs_stream_t stream) {
  return vfs_bn_reduce_partials_launch(partial, sums, scratch, G, bpg, C, stream_of(stream));
}
int vfs_bn_finalize(const double* sums, const float* gamma, const float* beta, float* bnp, float* running_mean,
                    float* running_var, int G, int C, double count, float eps, float momentum, vfs_stream_t stream) {
  return vfs_bn_finalize_launch(sums, gamma, beta, bnp, running_mean, running_var, G, C, count, eps, momentum, stream_of(stream));
}
int vfs_bn_stats_finalize(const float* partial, double* sums, double* scratch, const float* gamma, const float* beta, float* bnp,
                          float* running_mean, float* running_var, int G, int bpg, int C, double count, float eps, float momentum,
                          vfs_stream_t stream) {
  return vfs_bn_reduce_fused_launch(0, partial, sums, scratch, G, bpg, C, gamma, beta, bnp, running_mean, running_var, count, eps,
                                    momentum, nullptr, nullptr, stream_of(stream));
}
int vfs_bn_stats_raw_finalize(const vfs_bf16* raw, double* sums, const float* gamma, const float* beta, float* bnp, float* running_mean,
                              float* running_var, int G, int rows_per_group, int C, double count, float eps, float momentum,
                              vfs_stream_t stream) {
  if (!raw || !sums || !gamma || !beta || !bnp) return vfs_set_error(VFS_ERR_ARG, "bn_stats_raw_finalize: null buffer");
  return vfs_bn_stats_raw_launch(raw, sums, G, rows_per_group, C, gamma, beta, bnp, running_mean, running_var, count, eps, momentum,
                                 stream_of(stream));
}
int vfs_linear_bn_act(const vfs_bf16* x, const vfs_bf16* wf, const float* bias, const float* gamma, const float* beta, vfs_bf16* raw,
                      vfs_bf16* act, float* bnp, double* sums, float* running_mean, float* running_var, int M, int K, int C, int mpg,
                      int relu, double count, float eps, float momentum, vfs_stream_t stream) {
  if (!x || !wf || !gamma || !beta || !raw || !act || !bnp || !sums) return vfs_set_error(VFS_ERR_ARG, "linear_bn_act: null buffer");
  if (mpg <= 0 || M % mpg) return vfs_set_error(VFS_ERR_SHAPE, "linear_bn_act: M % mpg");
  LinBnArgs a{};
  a.x = x; a.w = wf; a.bias = bias; a.gamma = gamma; a.beta = beta; a.raw = raw; a.act = act; a.bnp = bnp; a.sums = sums;
  a.rm = running_mean; a.rv = running_var; a.M = M; a.K = K; a.C = C; a.G = M / mpg; a.mpg = mpg; a.relu = relu; a.count = count;
  a.eps = eps; a.momentum = momentum;
  return vfs_linear_bn_act_launch(a, stream_of(stream));
}
int vfs_bn_bwd_sums_paramgrad(const float* partial, double* sums, double* scratch, float* dgamma, float* dbeta, int G, int bpg,
                              int C, vfs_stream_t stream) {
  return vfs_bn_reduce_fused_launch(1, partial, sums, scratch, G, bpg, C, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0, 0.f, 0.f,
                                    dgamma, dbeta, stream_of(stream));
}
int vfs_bn_eval_params(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float* bnp,
                       int C, float eps, vfs_stream_t stream) {
  return vfs_bn_eval_params_launch(gamma, beta, running_mean, running_var, bnp, C, eps, stream_of(stream));
}
int vfs_bn_act_mask(const vfs_bf16* x, const float* bnp, const vfs_bf16* res, const vfs_bf16* rres, const float* rbnp, vfs_bf16* y,
                    uint8_t* mask_bits, long long M, int C, int mpg, int relu, vfs_stream_t stream) {
  return vfs_bn_act_launch(bn_act_args(x, bnp, res, rres, rbnp, y, mask_bits, M, C, mpg, relu), stream_of(stream));
}
int vfs_bn_act(const vfs_bf16* x, const float* bnp, const vfs_bf16* res, const vfs_bf16* rres, const float* rbnp, vfs_bf16* y,
               long long M, int C, int mpg, int relu, vfs_stream_t stream) {
  return vfs_bn_act_mask(x, bnp, res, rres, rbnp, y, nullptr, M, C, mpg, relu, stream);
}
int vfs_bn_act_fin_mask(const vfs_bf16* x, const float* partial, int bpg, const float* gamma, const float* beta, float* bnp, double* sums,
                        float* running_mean, float* running_var, const vfs_bf16* res, const vfs_bf16* rres, const float* rbnp, vfs_bf16* y,
                        uint8_t* mask_bits, long long M, int C, int mpg, int relu, double count, float eps, float momentum,
                        vfs_stream_t stream) {
  if (mpg <= 0 || M % mpg) return vfs_set_error(VFS_ERR_SHAPE, "bn_act_fin: M % mpg");
  const BnActArgs a = bn_act_args(x, bnp, res, rres, rbnp, y, mask_bits, M, C, mpg, relu);
  const BnFin f = bn_fin_fwd(partial, bpg, (int)(M / mpg), gamma, beta, bnp, sums, running_mean, running_var, count, eps, momentum);
  return vfs_bn_act_fin_launch(a, f, stream_of(stream));
}
int vfs_bn_act_fin_xchg(const vfs_bf16* x, const float* partial, int bpg, const float* gamma, const float* beta, float* bnp, double* sums,
                        float* running_mean, float* running_var, const vfs_bf16* res, const vfs_bf16* rres, const float* rbnp, vfs_bf16* y,
                        uint8_t* mask_bits, long long M, int C, int mpg, int relu, double count, float eps, float momentum,
                        const void* peers, int rank, int world, void* state, long long spin_limit, int seq, vfs_stream_t stream) {
  if (mpg <= 0 || M % mpg) return vfs_set_error(VFS_ERR_SHAPE, "bn_act_fin_xchg: M % mpg");
  if (int rc = xchg_check("bn_act_fin_xchg", seq, peers, state, partial)) return rc;
  const BnActArgs a = bn_act_args(x, bnp, res, rres, rbnp, y, mask_bits, M, C, mpg, relu);
  BnFin f = bn_fin_fwd(partial, bpg, (int)(M / mpg), gamma, beta, bnp, sums, running_mean, running_var, count, eps, momentum);
  f.x = make_tail(peers, rank, world, state, spin_limit, seq);
  return vfs_bn_act_fin_launch(a, f, stream_of(stream));
}
int vfs_bn_bwd_apply_fin_xchg(const vfs_bf16* g, const vfs_bf16* y, const vfs_bf16* x, const float* bnp, const float* partial, int bpg,
                              double* sums, float* dgamma, float* dbeta, vfs_bf16* dx, vfs_bf16* gm, long long M, int C, int mpg,
                              double count, int relu, const void* peers, int rank, int world, void* state, long long spin_limit,
                              int seq, vfs_stream_t stream) {
  if (mpg <= 0 || M % mpg) return vfs_set_error(VFS_ERR_SHAPE, "bn_bwd_apply_fin_xchg: M % mpg");
  if (int rc = xchg_check("bn_bwd_apply_fin_xchg", seq, peers, state, partial)) return rc;
  const BnBwdArgs a = bn_bwd_args(g, y, x, bnp, dx, gm, M, C, mpg, count, relu);
  BnFin f = bn_fin_bwd(partial, bpg, (int)(M / mpg), sums, dgamma, dbeta);
  f.x = make_tail(peers, rank, world, state, spin_limit, seq);
  return vfs_bn_bwd_apply_fin_launch(a, f, stream_of(stream));
}
int vfs_p2p_chain_start(void* state, vfs_stream_t stream) {
  if (!state) return vfs_set_error(VFS_ERR_ARG, "p2p_chain_start: null state");
  return vfs_p2p_chain_start_launch((unsigned long long*)state, stream_of(stream));
}
int vfs_bn_act_fin(const vfs_bf16* x, const float* partial, int bpg, const float* gamma, const float* beta, float* bnp, double* sums,
                   float* running_mean, float* running_var, const vfs_bf16* res, const vfs_bf16* rres, const float* rbnp, vfs_bf16* y,
                   long long M, int C, int mpg, int relu, double count, float eps, float momentum, vfs_stream_t stream) {
  return vfs_bn_act_fin_mask(x, partial, bpg, gamma, beta, bnp, sums, running_mean, running_var, res, rres, rbnp, y, nullptr, M, C, mpg,
                             relu, count, eps, momentum, stream);
}
int vfs_bn_relu_maxpool(const vfs_bf16* x, const float* bnp, vfs_bf16* y, uint8_t* idx, vfs_bf16* xpool, int N, int H, int W, int C,
                        int Hp, int Wp, int npg, vfs_stream_t stream) {
  BnPoolArgs a{};
  a.x = x; a.bnp = bnp; a.y = y; a.idx = idx; a.xpool = xpool; a.N = N; a.H = H; a.W = W; a.C = C; a.Hp = Hp; a.Wp = Wp; a.npg = npg;
  return vfs_bn_relu_maxpool_launch(a, stream_of(stream));
}
int vfs_maxpool_relu_bwd(const vfs_bf16* gp, const vfs_bf16* yp, const uint8_t* idx, vfs_bf16* ga, int N, int H, int W, int C,
                         int Hp, int Wp, vfs_stream_t stream) {
  PoolBwdArgs a{};
  a.gp = gp; a.yp = yp; a.idx = idx; a.ga = ga; a.N = N; a.H = H; a.W = W; a.C = C; a.Hp = Hp; a.Wp = Wp;
  return vfs_maxpool_relu_bwd_launch(a, stream_of(stream));
}
int vfs_bn_bwd_reduce(const vfs_bf16* g, const vfs_bf16* y, const vfs_bf16* x, const float* bnp, float* partial, long long M,
                      int C, int mpg, int ppb, int relu, vfs_stream_t stream) {
  if (ppb <= 0 || mpg % ppb) return vfs_set_error(VFS_ERR_SHAPE, "bn_bwd_reduce: pixels-per-group % pixels-per-block");
  BnBwdArgs a = bn_bwd_args(g, y, x, bnp, nullptr, nullptr, M, C, mpg, 0.0, relu);
  a.partial = partial; a.ppb = ppb;
  return vfs_bn_bwd_reduce_launch(a, (int)((M + ppb - 1) / ppb), stream_of(stream));
}
int vfs_bn_bwd_apply(const vfs_bf16* g, const vfs_bf16* y, const vfs_bf16* x, const float* bnp, const double* sums,
                     vfs_bf16* dx, vfs_bf16* gm, long long M, int C, int mpg, double count, int relu, vfs_stream_t stream) {
  BnBwdArgs a = bn_bwd_args(g, y, x, bnp, dx, gm, M, C, mpg, count, relu);
  a.sums = sums;
  return vfs_bn_bwd_apply_launch(a, stream_of(stream));
}
int vfs_bn_bwd_apply_fin(const vfs_bf16* g, const vfs_bf16* y, const vfs_bf16* x, const float* bnp, const float* partial, int bpg,
                         double* sums, float* dgamma, float* dbeta, vfs_bf16* dx, vfs_bf16* gm, long long M, int C, int mpg,
                         double count, int relu, vfs_stream_t stream) {
  if (mpg <= 0 || M % mpg) return vfs_set_error(VFS_ERR_SHAPE, "bn_bwd_apply_fin: M % mpg");
  const BnBwdArgs a = bn_bwd_args(g, y, x, bnp, dx, gm, M, C, mpg, count, relu);
  const BnFin f = bn_fin_bwd(partial, bpg, (int)(M / mpg), sums, dgamma, dbeta);
  return vfs_bn_bwd_apply_fin_launch(a, f, stream_of(stream));
}
int vfs_bn_bwd_apply_raw(const vfs_bf16* g, const vfs_bf16* y, const vfs_bf16* x, const float* bnp, double* sums, float* dgamma,
                         float* dbeta, vfs_bf16* dx, vfs_bf16* gm, long long M, int C, int mpg, double count, int relu,
                         vfs_stream_t stream) {
  if (mpg <= 0 || M % mpg) return vfs_set_error(VFS_ERR_SHAPE, "bn_bwd_apply_raw: M % mpg");
  int gcd = mpg, r = 512;      // ONE statistics row per group: the shapes the two-launch form serves with ppb == mpg (gcd(mpg, 512) == mpg or < 16)
  while (r) { const int q = gcd % r; gcd = r; r = q; }
  if (mpg > 512 || !(gcd == mpg || gcd < 16)) return vfs_set_error(VFS_ERR_SHAPE, "bn_bwd_apply_raw: one statistics row per group (mpg <= 512 and gcd(mpg, 512) == mpg or < 16)");
  BnBwdArgs a = bn_bwd_args(g, y, x, bnp, dx, gm, M, C, mpg, count, relu);
  a.ppb = mpg;
  const BnFin f = bn_fin_bwd(nullptr, 1, (int)(M / mpg), sums, dgamma, dbeta);
  return vfs_bn_bwd_apply_raw_launch(a, f, stream_of(stream));
}
int vfs_stem_pool_bn_bwd_reduce(const vfs_bf16* gp, const vfs_bf16* yp, const uint8_t* idx, const vfs_bf16* x, const vfs_bf16* xpool,
                                const float* bnp, float* partial, int N, int H, int W, int C, int Hp, int Wp, int npg, int ppb,
                                vfs_stream_t stream) {
  const long long mpg = (long long)npg * Hp * Wp;
  if (ppb <= 0 || mpg % ppb) return vfs_set_error(VFS_ERR_SHAPE, "stem_pool_bn_bwd_reduce: pooled pixels per group % ppb");
  if (!gp || !idx || !bnp || !partial || (!x && !xpool) || (!xpool && !yp)) return vfs_set_error(VFS_ERR_ARG, "stem_pool_bn_bwd_reduce: null buffer");
  StemBwdArgs a = stem_bwd_args(gp, yp, idx, x, bnp, N, H, W, C, Hp, Wp, npg);
  a.xp = xpool; a.partial = partial; a.ppb = ppb;
  const long long P = (long long)N * Hp * Wp;
  return vfs_stem_pool_bn_bwd_reduce_launch(a, (int)((P + ppb - 1) / ppb), stream_of(stream));
}
int vfs_stem_pool_bn_bwd_apply(const vfs_bf16* gp, const vfs_bf16* yp, const uint8_t* idx, const vfs_bf16* x, const float* bnp,
                               const double* sums, vfs_bf16* dx, int N, int H, int W, int C, int Hp, int Wp, int npg,
                               double count, vfs_stream_t stream) {
  StemBwdArgs a = stem_bwd_args(gp, yp, idx, x, bnp, N, H, W, C, Hp, Wp, npg);
  a.sums = sums; a.dx = dx; a.count = count;
  return vfs_stem_pool_bn_bwd_apply_launch(a, stream_of(stream));
}
int vfs_stem_wgrad_fused(const vfs_bf16* x4, const vfs_bf16* xraw, const vfs_bf16* gp, const vfs_bf16* yp, const uint8_t* idx,
                         const float* bnp, const double* sums, float* partial, float* grad, int N, int Hin, int Win, int Ho,
                         int Wo, int Hp, int Wp, int npg, double count, int nblocks, vfs_stream_t stream) {
  StemBwdArgs a = stem_bwd_args(gp, yp, idx, xraw, bnp, N, Ho, Wo, 64, Hp, Wp, npg);
  a.sums = sums; a.count = count;
  if ((size_t)N * Hin * Win * 8 >= 0xFFFFFFF0ull) return vfs_set_error(VFS_ERR_SHAPE, "stem_wgrad_fused: input >= 4 GiB");
  int rc = vfs_stem_wgrad_fused_launch(a, x4, Hin, Win, partial, nblocks, stream_of(stream));
  if (rc || !grad) return rc;
  return vfs_wgrad_reduce_launch(partial, grad, nblocks, 64, 224, 3, 7, 7, 1, stream_of(stream));
}
int vfs_bn_param_grad(const double* sums, float* dgamma, float* dbeta, int G, int C, vfs_stream_t stream) {
  return vfs_bn_param_grad_launch(sums, dgamma, dbeta, G, C, stream_of(stream));
}

int vfs_avgpool_fwd(const vfs_bf16* x, vfs_bf16* y, int N, int HW, int C, vfs_stream_t stream) {
  return vfs_avgpool_fwd_launch(x, y, N, HW, C, stream_of(stream));
}
int vfs_avgpool_bwd(const vfs_bf16* g, vfs_bf16* gx, int N, int HW, int C, vfs_stream_t stream) {
  return vfs_avgpool_bwd_launch(g, gx, N, HW, C, stream_of(stream));
}

int vfs_nhwc_bf16_to_nchw_f32(const vfs_bf16* src, float* dst, int N, int HW, int C, vfs_stream_t stream) {
  return vfs_nhwc_bf16_to_nchw_f32_launch(src, dst, N, HW, C, stream_of(stream));
}
int vfs_nchw_f32_to_nhwc_bf16(const float* src, vfs_bf16* dst, int N, int HW, int C, vfs_stream_t stream) {
  return vfs_nchw_f32_to_nhwc_bf16_launch(src, dst, N, HW, C, stream_of(stream));
}
int vfs_nchw_f32_add_nhwc_bf16(const float* src, const vfs_bf16* acc, vfs_bf16* dst, int N, int HW, int C, vfs_stream_t stream) {
  return vfs_nchw_f32_add_nhwc_bf16_launch(src, acc, dst, N, HW, C, stream_of(stream));
}
int vfs_bf16_add(const vfs_bf16* a, const vfs_bf16* b, vfs_bf16* dst, long long n, vfs_stream_t stream) {
  return vfs_bf16_add_launch(a, b, dst, n, stream_of(stream));
}

int vfs_cosine_loss_fwd(const vfs_bf16* p1, const vfs_bf16* z1, const vfs_bf16* p2, const vfs_bf16* z2, float* loss, int N,
                        int C, int T, int K, int negative, float weight, vfs_stream_t stream) {
  if (N % T) return vfs_set_error(VFS_ERR_SHAPE, "cosine_loss: N % T");
  LossArgs a = loss_args(p1, z1, p2, z2, N, C, T, K, negative, weight);
  a.loss = loss;
  return vfs_cosine_loss_fwd_launch(a, stream_of(stream));
}
int vfs_xcorr_fwd(const vfs_bf16* z, const vfs_bf16* x, float* out, int nz, int nx, int Hz, int Wz, int H, int W, int C, float scale,
                  vfs_stream_t stream) {
  if (!z || !x || !out) return vfs_set_error(VFS_ERR_ARG, "xcorr_fwd: null buffer");
  XcorrArgs a{};
  a.z = z; a.x = x; a.out = out; a.nz = nz; a.nx = nx; a.Hz = Hz; a.Wz = Wz; a.H = H; a.W = W; a.C = C; a.scale = scale;
  return vfs_xcorr_fwd_launch(a, stream_of(stream));
}
int vfs_xcorr_bwd(const vfs_bf16* z, const vfs_bf16* x, const float* g, vfs_bf16* dz, vfs_bf16* dx, int nz, int nx, int Hz, int Wz, int H, int W,
                  int C, float scale, vfs_stream_t stream) {
  if (!z || !x || !g || (!dz && !dx)) return vfs_set_error(VFS_ERR_ARG, "xcorr_bwd: null buffer");
  XcorrBwdArgs a{};
  a.z = z; a.x = x; a.g = g; a.dz = dz; a.dx = dx; a.nz = nz; a.nx = nx; a.Hz = Hz; a.Wz = Wz; a.H = H; a.W = W; a.C = C; a.scale = scale;
  return vfs_xcorr_bwd_launch(a, stream_of(stream));
}
int vfs_siamfc_loss(const float* responses, const float* labels, float* loss, float* grad, int n, int mode, float param, float scale,
                    vfs_stream_t stream) {
  if (!responses || !labels || !loss) return vfs_set_error(VFS_ERR_ARG, "siamfc_loss: null buffer");
  return vfs_siamfc_loss_launch(responses, labels, loss, grad, n, mode, param, scale, stream_of(stream));
}
int vfs_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int step, vfs_stream_t stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq) return vfs_set_error(VFS_ERR_ARG, "adam_step: null buffer");
  return vfs_adam_launch(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, stream_of(stream));
}
int vfs_siamfc_crops(const uint8_t* frame, const int* params, float* out, int H, int W, int S, int out_size, vfs_stream_t stream) {
  if (!frame || !params || !out) return vfs_set_error(VFS_ERR_ARG, "siamfc_crops: null buffer");
  if (S < 1 || S > VFS_SIAMFC_MAX_SCALES) return vfs_set_error(VFS_ERR_SHAPE, "siamfc_crops: 1 <= S <= 8");
  SiamCropArgs a{};
  a.frame = frame; a.out = out; a.H = H; a.W = W; a.S = S; a.out_size = out_size;
  for (int i = 0; i < S; ++i) {      // params is HOST memory: it travels as kernel arguments
    const int* p = params + 12 * i;
    SiamCropScale& c = a.sc[i];
    c.valid = p[0]; c.px0 = p[1]; c.py0 = p[2]; c.iw = p[3]; c.ih = p[4]; c.ow = p[5]; c.oh = p[6]; c.padx = p[7]; c.pady = p[8];
    c.fill[0] = p[9]; c.fill[1] = p[10]; c.fill[2] = p[11];
    if (c.valid && c.ow > 0 && c.oh > 0) { c.sx = (double)c.iw / (double)c.ow; c.sy = (double)c.ih / (double)c.oh; }
  }
  return vfs_siamfc_crops_launch(a, stream_of(stream));
}
int vfs_siamfc_upsample(const float* responses, const int* tap_idx, const float* tap_w, const float* penalty, float* up_out,
                        unsigned long long* scale_max, int S, int r, int up, vfs_stream_t stream) {
  if (!responses || !tap_idx || !tap_w || !penalty || !up_out || !scale_max) return vfs_set_error(VFS_ERR_ARG, "siamfc_upsample: null buffer");
  if (((size_t)tap_idx | (size_t)tap_w) & 15) return vfs_set_error(VFS_ERR_ARG, "siamfc_upsample: the tap tables must be 16-byte aligned");
  return vfs_siamfc_upsample_launch(responses, tap_idx, tap_w, penalty, up_out, scale_max, S, r, up, stream_of(stream));
}
int vfs_siamfc_peak(const float* up_in, const unsigned long long* scale_max, const double* hann, int* record, int S, int up,
                    float one_minus_wi, double window_influence, vfs_stream_t stream) {
  if (!up_in || !scale_max || !hann || !record) return vfs_set_error(VFS_ERR_ARG, "siamfc_peak: null buffer");
  return vfs_siamfc_peak_launch(up_in, scale_max, hann, record, S, up, one_minus_wi, window_influence, stream_of(stream));
}
int vfs_siamfc_batch_crops(const uint8_t* frames, const long long* frame_off, const double* state, int* meta, const double* factors, float* out,
                           int N, int S, int out_size, int use_z, vfs_stream_t stream) {
  SiamBatchCropArgs a{};      // every check (null buffers, alignment, sizes) before the launch: vfs_siamfc_batch_crops_check, siamfc_batch.h
  a.frames = frames; a.frame_off = frame_off; a.state = state; a.meta = meta; a.factors = factors; a.out = out;
  a.N = N; a.S = S; a.out_size = out_size; a.use_z = use_z;
  return vfs_siamfc_batch_crops_launch(a, stream_of(stream));
}
int vfs_siamfc_batch_upsample(const float* responses, const int* tap_idx, const float* tap_w, const float* penalty, float* up_out,
                              unsigned long long* scale_max, int N, int S, int r, int up, vfs_stream_t stream) {
  return vfs_siamfc_batch_upsample_launch(responses, tap_idx, tap_w, penalty, up_out, scale_max, N, S, r, up, stream_of(stream));
}
int vfs_siamfc_batch_peak(const float* up_in, const unsigned long long* scale_max, const double* hann, const double* factors, double* state,
                          int* meta, double* boxes, int* records, long long rows_cap, int N, int S, int up, float one_minus_wi,
                          double window_influence, double total_stride, double response_up, double instance_sz, double scale_lr,
                          vfs_stream_t stream) {
  SiamBatchPeakArgs a{};
  a.up_in = up_in; a.scale_max = scale_max; a.hann = hann; a.factors = factors; a.state = state; a.meta = meta; a.boxes = boxes;
  a.records = records; a.rows_cap = rows_cap; a.N = N; a.S = S; a.up = up; a.one_minus_wi = one_minus_wi; a.wi = window_influence;
  a.total_stride = total_stride; a.response_up = response_up; a.instance_sz = instance_sz; a.scale_lr = scale_lr;
  return vfs_siamfc_batch_peak_launch(a, stream_of(stream));
}
int vfs_loss_means(const float* loss, float* means, int K, int N, vfs_stream_t stream) {
  if (!loss || !means) return vfs_set_error(VFS_ERR_ARG, "loss_means: null buffer");
  return vfs_loss_means_launch(loss, means, K, N, stream_of(stream));
}
int vfs_cosine_loss_bwd(const vfs_bf16* p1, const vfs_bf16* z1, const vfs_bf16* p2, const vfs_bf16* z2, const float* gloss,
                        vfs_bf16* dp1, vfs_bf16* dp2, int N, int C, int T, int K, int negative, float weight,
                        vfs_stream_t stream) {
  if (N % T) return vfs_set_error(VFS_ERR_SHAPE, "cosine_loss: N % T");
  LossArgs a = loss_args(p1, z1, p2, z2, N, C, T, K, negative, weight);
  a.gloss = gloss; a.dp1 = dp1; a.dp2 = dp2;
  return vfs_cosine_loss_bwd_launch(a, stream_of(stream));
}

int vfs_dense_cosine_loss_workspace_bytes(int N, int S, int C, int K, long long* bytes) {
  if (!bytes) return vfs_set_error(VFS_ERR_ARG, "dense_cosine_loss_workspace_bytes: null");
  if (N < 1 || S < 1 || K < 1 || C < 8 || C % 8 || C > VFS_DENSE_LOSS_MAX_C)
    return vfs_set_error(VFS_ERR_SHAPE, "dense_cosine_loss_workspace_bytes: N, S, K >= 1, C % 8 == 0, C <= 2048");
  *bytes = dense_loss_workspace_need(N, S, C, K);
  return VFS_OK;
}
int vfs_dense_cosine_loss_fwd(const vfs_bf16* p1, const vfs_bf16* z1, const vfs_bf16* p2, const vfs_bf16* z2, float* loss, void* workspace,
                              long long workspace_bytes, int N, int S, int C, int T, int K, int negative, float weight,
                              vfs_stream_t stream) {
  if (int rc = dense_loss_check("dense_cosine_loss_fwd", p1, z1, p2, z2, N, S, C, T, K)) return rc;
  if (!loss) return vfs_set_error(VFS_ERR_ARG, "dense_cosine_loss_fwd: null loss");
  if (!workspace || workspace_bytes < dense_loss_workspace_need(N, S, C, K))
    return vfs_set_error(VFS_ERR_ARG, "dense_cosine_loss_fwd: workspace smaller than vfs_dense_cosine_loss_workspace_bytes(N, S, C, K)");
  DenseLossArgs a = dense_loss_args(p1, z1, p2, z2, N, S, C, T, K, negative, weight);
  a.loss = loss; a.partial = (float*)workspace;
  return vfs_dense_cosine_loss_fwd_launch(a, stream_of(stream));
}
int vfs_dense_cosine_loss_bwd(const vfs_bf16* p1, const vfs_bf16* z1, const vfs_bf16* p2, const vfs_bf16* z2, const float* gloss,
                              vfs_bf16* dp1, vfs_bf16* dp2, int N, int S, int C, int T, int K, int negative, float weight,
                              vfs_stream_t stream) {
  if (int rc = dense_loss_check("dense_cosine_loss_bwd", p1, z1, p2, z2, N, S, C, T, K)) return rc;
  if (!gloss || !dp1 || !dp2 || (((size_t)dp1 | (size_t)dp2) & 15)) return vfs_set_error(VFS_ERR_ARG, "dense_cosine_loss_bwd: null or unaligned gradient buffer");
  DenseLossArgs a = dense_loss_args(p1, z1, p2, z2, N, S, C, T, K, negative, weight);
  a.gloss = gloss; a.dp1 = dp1; a.dp2 = dp2;
  return vfs_dense_cosine_loss_bwd_launch(a, stream_of(stream));
}

int vfs_bn_reduce_partials_xchg(const float* partial, double* sums, double* scratch, int G, int bpg, int C, const void* peers, int rank,
                                int world, void* state, long long spin_limit, vfs_stream_t stream) {
  if (!partial || !sums || !peers || !state || spin_limit <= 0) return vfs_set_error(VFS_ERR_ARG, "bn_reduce_partials_xchg: bad argument");
  const P2PTail x = make_tail(peers, rank, world, state, spin_limit);
  return vfs_bn_reduce_partials_launch(partial, sums, scratch, G, bpg, C, stream_of(stream), &x);
}
int vfs_bn_bwd_sums_paramgrad_xchg(const float* partial, double* sums, double* scratch, float* dgamma, float* dbeta, int G, int bpg, int C,
                                   const void* peers, int rank, int world, void* state, long long spin_limit, vfs_stream_t stream) {
  if (!partial || !sums || !peers || !state || spin_limit <= 0) return vfs_set_error(VFS_ERR_ARG, "bn_bwd_sums_paramgrad_xchg: bad argument");
  const P2PTail x = make_tail(peers, rank, world, state, spin_limit);
  return vfs_bn_reduce_fused_launch(1, partial, sums, scratch, G, bpg, C, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0, 0.f, 0.f,
                                    dgamma, dbeta, stream_of(stream), &x);
}
int vfs_p2p_window_bytes(long long* bytes, int* max_doubles, int* max_world) {
  if (!bytes || !max_doubles || !max_world) return vfs_set_error(VFS_ERR_ARG, "p2p_window_bytes: null");
  return vfs_p2p_window_bytes_host(bytes, max_doubles, max_world);
}
int vfs_p2p_alloc(void** window) { return window ? vfs_p2p_alloc_host(window) : vfs_set_error(VFS_ERR_ARG, "p2p_alloc: null"); }
int vfs_p2p_free(void* window) { return window ? vfs_p2p_free_host(window) : VFS_OK; }
int vfs_p2p_export(void* window, void* handle64) {
  return (window && handle64) ? vfs_p2p_export_host(window, handle64) : vfs_set_error(VFS_ERR_ARG, "p2p_export: null");
}
int vfs_p2p_import(const void* handle64, void** window) {
  return (window && handle64) ? vfs_p2p_import_host(handle64, window) : vfs_set_error(VFS_ERR_ARG, "p2p_import: null");
}
int vfs_p2p_unimport(void* window) { return window ? vfs_p2p_unimport_host(window) : VFS_OK; }
int vfs_p2p_allreduce_f64(double* buf, int n, const void* peers, int rank, int world, void* state, int phase, long long spin_limit,
                          vfs_stream_t stream) {
  if (!buf || !peers || !state || !(phase & 3) || spin_limit <= 0) return vfs_set_error(VFS_ERR_ARG, "p2p_allreduce_f64: bad argument");
  return vfs_p2p_allreduce_f64_launch(buf, n, reinterpret_cast<void* const*>(peers), rank, world,
                                      reinterpret_cast<unsigned long long*>(state), phase, (unsigned long long)spin_limit, stream_of(stream));
}

int vfs_simloss_colnorm(const float* x, float* inv, int B, int C, int S, vfs_stream_t stream) {
  if (!x || !inv || B <= 0 || C <= 0 || S <= 0) return vfs_set_error(VFS_ERR_ARG, "simloss_colnorm: bad argument");
  return vfs_simloss_colnorm_launch(x, inv, B, C, S, stream_of(stream));
}
int vfs_simloss_fwd(const float* a, const float* l, const float* inva, const float* invl, const float* mask, float* partial, float* loss,
                    int B, int C, int Sa, int Sl, int pairwise, int negative, float weight, vfs_stream_t stream) {
  if (!a || !l || !partial || !loss || B <= 0 || C <= 0 || Sa <= 0 || Sl <= 0) return vfs_set_error(VFS_ERR_ARG, "simloss_fwd: bad argument");
  if (!pairwise && Sa != Sl) return vfs_set_error(VFS_ERR_SHAPE, "simloss_fwd: non-pairwise operands must have the same positions");
  if (!pairwise && mask) return vfs_set_error(VFS_ERR_ARG, "simloss_fwd: a mask needs pairwise (sim_loss.py:46-47)");
  return vfs_simloss_fwd_launch(a, l, inva, invl, mask, partial, loss, B, C, Sa, Sl, pairwise, negative, weight, stream_of(stream));
}
int vfs_simloss_bwd(const float* other, const float* invo, const float* mask, int mask_transposed, const float* gloss, float* d, int B,
                    int C, int Sself, int Sother, int pairwise, int negative, float weight, vfs_stream_t stream) {
  if (!other || !gloss || !d || B <= 0 || C <= 0 || Sself <= 0 || Sother <= 0) return vfs_set_error(VFS_ERR_ARG, "simloss_bwd: bad argument");
  if (!pairwise && Sself != Sother) return vfs_set_error(VFS_ERR_SHAPE, "simloss_bwd: non-pairwise operands must have the same positions");
  return vfs_simloss_bwd_launch(other, invo, mask, mask_transposed, gloss, d, B, C, Sself, Sother, pairwise, negative, weight, stream_of(stream));
}
int vfs_simloss_norm_bwd(const float* x, const float* inv, const float* d, float* dx, int B, int C, int S, vfs_stream_t stream) {
  if (!x || !d || !dx || B <= 0 || C <= 0 || S <= 0) return vfs_set_error(VFS_ERR_ARG, "simloss_norm_bwd: bad argument");
  return vfs_simloss_norm_bwd_launch(x, inv, d, dx, B, C, S, stream_of(stream));
}

// masked_attention (attn_train.hip): the limits of the kernels, shared by the three entry points
static int attn_shape(const char* who, AttnShape& s, int N, int C, int T, int H, int W, int CO, int neighbor_range, int topk, float temperature,
                      int normalize) {
  if (N < 1 || N > 65535 || H < 1 || W < 1) return fail(VFS_ERR_SHAPE, who, "1 <= N <= 65535, H >= 1, W >= 1");
  if (topk < 1 || topk > VFS_ATTN_MAX_TOPK) return fail(VFS_ERR_SHAPE, who, "1 <= topk <= 10");
  if (neighbor_range != 0 && neighbor_range < 2) return fail(VFS_ERR_SHAPE, who, "neighbor_range >= 2, or 0 for no window");
  if (C < 64 || C % 64 || C > VFS_ATTN_MAX_C) return fail(VFS_ERR_SHAPE, who, "C % 64 == 0 and C <= 2048");
  if (T < 1 || T > VFS_ATTN_MAX_T) return fail(VFS_ERR_SHAPE, who, "1 <= T <= 64");
  if (CO < 1 || CO > VFS_ATTN_MAX_CO) return fail(VFS_ERR_SHAPE, who, "1 <= CO <= 256");
  if ((long long)T * H * W >= (1ll << 31)) return fail(VFS_ERR_SHAPE, who, "T * H * W < 2^31");
  if (!(temperature > 0.0f) || !(temperature < INFINITY)) return fail(VFS_ERR_ARG, who, "temperature must be positive and finite");
  s.N = N; s.C = C; s.T = T; s.H = H; s.W = W; s.CO = CO; s.neighbor_range = neighbor_range; s.topk = topk; s.temperature = temperature;
  s.normalize = normalize != 0;
  return VFS_OK;
}
int vfs_masked_attention_workspace_bytes(int N, int C, int T, int H, int W, int CO, int topk, int normalize, long long* bytes) {
  AttnShape s;
  if (!bytes) return vfs_set_error(VFS_ERR_ARG, "masked_attention_workspace_bytes: null out-pointer");
  const int rc = attn_shape("masked_attention_workspace_bytes", s, N, C, T, H, W, CO, 0, topk, 1.0f, normalize);
  if (rc) return rc;
  *bytes = 4 * vfs_attn_bwd_workspace_floats(s, true, true);
  return VFS_OK;
}
int vfs_masked_attention_fwd(const float* query, const float* key, const float* value, float* out, int* idx, float* weights, float* invq,
                             float* invk, int N, int C, int T, int H, int W, int CO, int neighbor_range, int topk, float temperature,
                             int normalize, vfs_stream_t stream) {
  AttnShape s;
  const int rc = attn_shape("masked_attention_fwd", s, N, C, T, H, W, CO, neighbor_range, topk, temperature, normalize);
  if (rc) return rc;
  if (!query || !key || !value || !out || !idx || !weights || (normalize && (!invq || !invk)))
    return vfs_set_error(VFS_ERR_ARG, "masked_attention_fwd: null buffer");
  return vfs_attn_fwd_launch(s, query, key, value, out, idx, weights, invq, invk, stream_of(stream));
}
int vfs_masked_attention_bwd(const float* query, const float* key, const float* value, const float* dout, const int* idx, const float* weights,
                             const float* invq, const float* invk, float* dq, float* dk, float* dv, void* workspace,
                             long long workspace_bytes, int N, int C, int T, int H, int W, int CO, int neighbor_range, int topk,
                             float temperature, int normalize, vfs_stream_t stream) {
  AttnShape s;
  const int rc = attn_shape("masked_attention_bwd", s, N, C, T, H, W, CO, neighbor_range, topk, temperature, normalize);
  if (rc) return rc;
  if (!query || !key || !value || !dout || !idx || !weights || (normalize && (!invq || !invk)))
    return vfs_set_error(VFS_ERR_ARG, "masked_attention_bwd: null buffer");
  if (!dq && !dk && !dv) return VFS_OK;
  if (!workspace || workspace_bytes < 4 * vfs_attn_bwd_workspace_floats(s, dq != nullptr, dk != nullptr))
    return vfs_set_error(VFS_ERR_ARG, "masked_attention_bwd: workspace smaller than vfs_masked_attention_workspace_bytes");
  return vfs_attn_bwd_launch(s, query, key, value, dout, idx, weights, invq, invk, dq, dk, dv, static_cast<float*>(workspace), stream_of(stream));
}

int vfs_sgd_step(float* params, const float* grads, float* momentum_buf, long long n, float lr, float momentum,
                 float weight_decay, const void* skip_flag, vfs_stream_t stream) {
  return vfs_sgd_launch(params, grads, momentum_buf, n, lr, momentum, weight_decay, nullptr, static_cast<const unsigned long long*>(skip_flag), stream_of(stream));
}
int vfs_scale(float* x, long long n, float scale, vfs_stream_t stream) { return vfs_scale_launch(x, n, scale, stream_of(stream)); }

// gradient clipping: norm_type is 2 or +infinity, as a float (what torch's clip_grad_norm_ takes)
static int grad_norm_type(const char* who, float norm_type, int* inf_norm) {
  if (norm_type == 2.0f) *inf_norm = 0;
  else if (norm_type == __builtin_inff()) *inf_norm = 1;
  else return fail(VFS_ERR_ARG, who, "norm_type must be 2 or infinity");
  return VFS_OK;
}
int vfs_grad_norm_rows(int* rows) {
  if (!rows) return vfs_set_error(VFS_ERR_ARG, "grad_norm_rows: bad argument");
  *rows = VFS_GRAD_NORM_ROWS;
  return VFS_OK;
}
int vfs_grad_norm_partial(const float* grads, long long n, float norm_type, double* partials, int accumulate, vfs_stream_t stream) {
  int inf_norm;
  if (!grads || !partials) return vfs_set_error(VFS_ERR_ARG, "grad_norm_partial: null buffer");
  if (n < 0) return vfs_set_error(VFS_ERR_ARG, "grad_norm_partial: n < 0");
  if ((size_t)grads & 15) return vfs_set_error(VFS_ERR_ARG, "grad_norm_partial: 16-byte aligned gradients");
  if (int rc = grad_norm_type("grad_norm_partial", norm_type, &inf_norm)) return rc;
  return vfs_grad_norm_partial_launch(grads, n, inf_norm, partials, accumulate, stream_of(stream));
}
int vfs_grad_norm_finish(const double* partials, float norm_type, double max_norm, float* out, vfs_stream_t stream) {
  int inf_norm;
  if (!partials || !out) return vfs_set_error(VFS_ERR_ARG, "grad_norm_finish: null buffer");
  if (int rc = grad_norm_type("grad_norm_finish", norm_type, &inf_norm)) return rc;
  if (!(max_norm > 0.0)) return vfs_set_error(VFS_ERR_ARG, "grad_norm_finish: max_norm <= 0");
  return vfs_grad_norm_finish_launch(partials, inf_norm, max_norm, out, stream_of(stream));
}
int vfs_sgd_step_clip(float* params, const float* grads, float* momentum_buf, long long n, float lr, float momentum,
                      float weight_decay, const float* clip, const void* skip_flag, vfs_stream_t stream) {
  if (!params || !grads || !momentum_buf || !clip) return vfs_set_error(VFS_ERR_ARG, "sgd_step_clip: null buffer");
  if (n < 0) return vfs_set_error(VFS_ERR_ARG, "sgd_step_clip: n < 0");
  return vfs_sgd_launch(params, grads, momentum_buf, n, lr, momentum, weight_decay, clip, static_cast<const unsigned long long*>(skip_flag), stream_of(stream));
}
// table-driven optimizer step: the map is built and checked on the host (opt_table.h), the step checks what it can see
int vfs_opt_segment_map_words(long long n, int nseg, long long* words) {
  if (!words || n < 0 || nseg < 0) return vfs_set_error(VFS_ERR_ARG, "opt_segment_map_words: bad argument");
  *words = vfs_opt_map_words_of(n, nseg);
  return VFS_OK;
}
int vfs_opt_segment_map(const long long* segments, int nseg, long long n, int ngroups, int* map, long long words) {
  if (const char* what = vfs_opt_map_build(segments, nseg, n, ngroups, map, words)) return fail(VFS_ERR_ARG, "opt_segment_map", what);
  return VFS_OK;
}
int vfs_opt_step_table(int kind, float* params, const float* grads, float* state1, float* state2, long long n, const int* map, int nseg,
                       const float* hyper, int ngroups, float* table, int nesterov, int step, const float* clip, const void* skip_flag,
                       vfs_stream_t stream) {
  if (const char* what = vfs_opt_step_check(kind, params, grads, state1, state2, n, map, nseg, hyper, ngroups, table, nesterov, step))
    return fail(VFS_ERR_ARG, "opt_step_table", what);
  return vfs_opt_table_launch(kind, params, grads, state1, state2, n, map, nseg, hyper, ngroups, table, nesterov, step, clip,
                              static_cast<const unsigned long long*>(skip_flag), stream_of(stream));
}
int vfs_scale_by(float* x, long long n, const float* coef, vfs_stream_t stream) {
  if (!x || !coef) return vfs_set_error(VFS_ERR_ARG, "scale_by: null buffer");
  if (n < 0) return vfs_set_error(VFS_ERR_ARG, "scale_by: n < 0");
  if ((size_t)x & 15) return vfs_set_error(VFS_ERR_ARG, "scale_by: 16-byte aligned buffer");
  return vfs_scale_by_launch(x, n, coef, stream_of(stream));
}
int vfs_f32_to_bf16(const float* src, vfs_bf16* dst, long long n, float scale, vfs_stream_t stream) {
  return vfs_f32_to_bf16_launch(src, dst, n, scale, stream_of(stream));
}
int vfs_bf16_to_f32(const vfs_bf16* src, float* dst, long long n, vfs_stream_t stream) { return vfs_bf16_to_f32_launch(src, dst, n, stream_of(stream)); }

int vfs_l2norm_rows(const vfs_bf16* x, vfs_bf16* y, long long P, int C, vfs_stream_t stream) {
  if (P < 1 || P > 4LL * 0x7fffffff || C < 1) return vfs_set_error(VFS_ERR_SHAPE, "l2norm_rows: P >= 1 (four rows per workgroup), C >= 1");
  if (!x || !y) return vfs_set_error(VFS_ERR_ARG, "l2norm_rows: null buffer");
  return vfs_l2norm_rows_launch(x, y, P, C, stream_of(stream));
}
int vfs_labelprop_workspace_bytes(int H, int W, long long* bytes) {
  if (!bytes || H <= 0 || W <= 0) return vfs_set_error(VFS_ERR_ARG, "labelprop_workspace_bytes: bad argument");
  *bytes = lp_workspace_need(H, W);
  return VFS_OK;
}
int vfs_labelprop(const vfs_bf16* fbank, const float* sbank, float* out, void* workspace, long long workspace_bytes, int qframe,
                  const int* kslot, int nkeys, int H, int W, int C, int CO, int radius, int non_mask_len, int topk, float temperature,
                  vfs_stream_t stream) {
  // the cheap refusals come before the workspace is looked at: nothing below may index with these
  if (H < 1 || W < 1 || C < 1 || CO < 1) return vfs_set_error(VFS_ERR_SHAPE, "labelprop: H, W, C, CO >= 1");
  if (topk < 1 || topk > 10) return vfs_set_error(VFS_ERR_SHAPE, "labelprop: 1 <= topk <= 10");
  if ((long long)H * W > 0x7fffffff / LP_MAX_KEYS) return vfs_set_error(VFS_ERR_SHAPE, "labelprop: nkeys * H * W must fit the int candidate ids");
  if (int rc = lp_check("labelprop", nkeys, radius, non_mask_len, true, workspace, workspace_bytes, H, W)) return rc;
  if (!fbank || !sbank || !out || !kslot) return vfs_set_error(VFS_ERR_ARG, "labelprop: null buffer");
  if (qframe < 0) return vfs_set_error(VFS_ERR_ARG, "labelprop: qframe >= 0");
  for (int i = 0; i < nkeys; ++i)
    if (kslot[i] < 0) return vfs_set_error(VFS_ERR_ARG, "labelprop: kslot entries >= 0");
  if (!(temperature > 0.f)) return vfs_set_error(VFS_ERR_ARG, "labelprop: temperature > 0");
  LabelPropArgs a{};
  a.fbank = fbank; a.sbank = sbank; a.out = out; a.qframe = qframe; a.nkeys = nkeys;
  a.pval = (float*)workspace; a.pidx = lp_pidx(workspace, H, W);
  lp_fill_kslot(a.kslot, kslot, nkeys);
  a.H = H; a.W = W; a.C = C; a.CO = CO; a.radius = radius; a.non_mask_len = non_mask_len; a.topk = topk; a.inv_temp = 1.0f / temperature;
  return vfs_labelprop_launch(a, stream_of(stream));
}
int vfs_seg_postprocess(const float* seg, float* partial, uint8_t* label, int H, int W, int CO, int Ho, int Wo,
                        vfs_stream_t stream) {
  if (H < 1 || W < 1 || Ho < 1 || Wo < 1 || CO < 1 || CO > LP_MAX_CLASSES)
    return vfs_set_error(VFS_ERR_SHAPE, "seg_postprocess: H, W, Ho, Wo >= 1, 1 <= classes <= 256");
  if ((long long)Ho * Wo > 0x7fffffff - 255 || (long long)H * W * CO > 0x7fffffff)
    return vfs_set_error(VFS_ERR_SHAPE, "seg_postprocess: Ho * Wo and H * W * classes must fit an int");
  if (!seg || !partial || !label) return vfs_set_error(VFS_ERR_ARG, "seg_postprocess: null buffer");
  return vfs_seg_postprocess_launch(seg, partial, label, H, W, CO, Ho, Wo, stream_of(stream));
}
int vfs_onehot(const uint8_t* labels, float* out, int P, int CO, vfs_stream_t stream) {
  if (P < 1 || CO < 1 || CO > LP_MAX_CLASSES) return vfs_set_error(VFS_ERR_SHAPE, "onehot: P >= 1, 1 <= classes <= 256");
  if ((long long)P * CO > 0x7fffffff - 255) return vfs_set_error(VFS_ERR_SHAPE, "onehot: P * classes must fit an int");
  if (!labels || !out) return vfs_set_error(VFS_ERR_ARG, "onehot: null buffer");
  return vfs_onehot_launch(labels, out, P, CO, stream_of(stream));
}

// ---- fp32 evaluation path (exact_f32.hip) ----
int vfs_conv_f32_fwd(const float* x, const float* w, const float* scale, const float* shift, const float* res, float* y, int N, int H,
                     int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int dilation, int relu,
                     vfs_stream_t stream) {
  if (!x || !w || !y) return vfs_set_error(VFS_ERR_ARG, "conv_f32_fwd: null buffer");
  ConvF32Args a{};
  a.x = x; a.w = w; a.scale = scale; a.shift = shift; a.res = res; a.y = y;
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Ho = Ho; a.Wo = Wo; a.Cout = Cout; a.KH = KH; a.KW = KW;
  a.stride = stride; a.pad = pad; a.dil = dilation; a.relu = relu;
  return vfs_conv_f32_launch(a, stream_of(stream));
}
int vfs_imgs_to_nhwc4_f32(const float* imgs, float* out, int B, int V, int T, int H, int W, vfs_stream_t stream) {
  return vfs_imgs_to_nhwc4_f32_launch(imgs, out, B, V, T, H, W, stream_of(stream));
}
int vfs_maxpool_f32(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo, vfs_stream_t stream) {
  return vfs_maxpool_f32_launch(x, y, N, H, W, C, Ho, Wo, stream_of(stream));
}
int vfs_l2norm_rows_f32(const float* x, float* y, long long P, int C, vfs_stream_t stream) {
  return vfs_l2norm_rows_f32_launch(x, y, P, C, stream_of(stream));
}
int vfs_labelprop_f32(const float* fbank, const float* sbank, float* out, void* workspace, long long workspace_bytes, int qframe,
                      const int* kslot, int nkeys, int H, int W, int C, int CO, int radius, int non_mask_len, int topk, float temperature,
                      vfs_stream_t stream) {
  if (int rc = lp_check("labelprop_f32", nkeys, radius, non_mask_len, true, workspace, workspace_bytes, H, W)) return rc;
  const LabelPropF32Args a = lp_f32_args(fbank, sbank, out, workspace, qframe, kslot, nkeys, H, W, C, CO, radius, non_mask_len, topk, temperature);
  return vfs_labelprop_f32_launch(a, stream_of(stream));
}
int vfs_split_rows_bf16x2(const float* x, vfs_bf16* hl, long long P, int C, vfs_stream_t stream) {
  if (!x || !hl) return vfs_set_error(VFS_ERR_ARG, "split_rows_bf16x2: null buffer");
  return vfs_split_rows_bf16x2_launch(x, hl, P, C, stream_of(stream));
}
static long long lp2_lists_bytes(int H, int W, int entries) { return (long long)entries * H * W * 8; }
static long long lp2_counts_bytes(int H, int W) { return ((long long)(LP2_MAX_SPLIT + 1) * H * W * 4 + 15) / 16 * 16; }      // counts + thresholds
// workspace: [dense kernel's partial lists][candidate lists: `entries` per query, shared out among the key-frame splits in use]
// [counts + thresholds][16 bytes of flags].  Round 6: the list area follows the workspace the caller passes (vfs_labelprop_f32_2pass
// derives the entries per query from workspace_bytes) - 4608 entries (237 MB at 60 x 107) is what never overflowed on the bench
// clips, fewer entries trade memory for dense redos of the first frames of a clip (cold thresholds, long lists).
int vfs_labelprop_f32_2pass_workspace_bytes_for(int H, int W, int entries_per_query, long long* bytes) {
  long long dense = 0;
  if (!bytes || entries_per_query < 16 || vfs_labelprop_workspace_bytes(H, W, &dense) != VFS_OK)
    return vfs_set_error(VFS_ERR_ARG, "labelprop_f32_2pass_workspace_bytes: bad argument (at least 16 list entries per query)");
  if (entries_per_query > LP2_MAX_SPLIT * LP2_MAX_CAP) entries_per_query = LP2_MAX_SPLIT * LP2_MAX_CAP;
  *bytes = dense + lp2_lists_bytes(H, W, entries_per_query) + lp2_counts_bytes(H, W) + 16;
  return VFS_OK;
}
int vfs_labelprop_f32_2pass_workspace_bytes(int H, int W, long long* bytes) {
  return vfs_labelprop_f32_2pass_workspace_bytes_for(H, W, LP2_MAX_SPLIT * LP2_MAX_CAP, bytes);
}
int vfs_labelprop_f32_2pass(const float* fbank, const vfs_bf16* hlbank, const float* sbank, float* out, void* workspace,
                            long long workspace_bytes, int qframe, const int* kslot, int nkeys, int H, int W, int C, int CO, int radius,
                            int non_mask_len, int topk, float temperature, int unit_rows, vfs_stream_t stream) {
  if (!hlbank || !unit_rows || !vfs_lp2_eligible(C) || (long long)H * W >= (1 << 21))      // (2^21 positions: the float index arithmetic of pass 1)
    return vfs_labelprop_f32(fbank, sbank, out, workspace, workspace_bytes, qframe, kslot, nkeys, H, W, C, CO, radius, non_mask_len, topk,
                             temperature, stream);
  if (int rc = lp_check("labelprop_f32_2pass", nkeys, radius, non_mask_len, false, workspace, workspace_bytes, H, W)) return rc;      // its workspace: below
  long long need = 0, dense = 0;
  if (vfs_labelprop_f32_2pass_workspace_bytes_for(H, W, 16, &need) != VFS_OK || vfs_labelprop_workspace_bytes(H, W, &dense) != VFS_OK || !workspace ||
      workspace_bytes < need)
    return vfs_set_error(VFS_ERR_ARG, "labelprop_f32_2pass: workspace smaller than vfs_labelprop_f32_2pass_workspace_bytes_for(H, W, 16)");
  Lp2Args p{};
  p.fbank = fbank; p.hl = hlbank; p.sbank = sbank; p.out = out;
  const long long entries = (workspace_bytes - dense - lp2_counts_bytes(H, W) - 16) / ((long long)H * W * 8);
  p.entries = (int)(entries > LP2_MAX_SPLIT * LP2_MAX_CAP ? LP2_MAX_SPLIT * LP2_MAX_CAP : entries);
  char* ws = (char*)workspace + dense;
  p.lists = (unsigned long long*)ws;
  p.counts = (int*)(ws + lp2_lists_bytes(H, W, p.entries));
  p.gthr = p.counts + (size_t)LP2_MAX_SPLIT * H * W;
  p.flags = (int*)(ws + lp2_lists_bytes(H, W, p.entries) + lp2_counts_bytes(H, W));
  p.qframe = qframe; p.nkeys = nkeys;
  lp_fill_kslot(p.kslot, kslot, nkeys);
  p.H = H; p.W = W; p.C = C; p.CO = CO; p.radius = radius; p.topk = topk; p.non_mask_len = non_mask_len; p.temperature = temperature;
  int rc = vfs_labelprop_f32_2pass_launch(p, stream_of(stream));
  if (rc) return rc;
  // the dense kernel as the overflow fallback: its workgroups read the flag and leave when no list overflowed
  LabelPropF32Args a = lp_f32_args(fbank, sbank, out, workspace, qframe, kslot, nkeys, H, W, C, CO, radius, non_mask_len, topk, temperature);
  a.run_flag = p.flags;
  return vfs_labelprop_f32_launch(a, stream_of(stream));
}
// ---- a batch of videos in lock-step: one call = one step of every slot (include/vfs_hip.h: banks, descriptor rows, workspace) ----
static long long lpb_round(long long bytes) { return (bytes + 255) / 256 * 256; }
static int lpb_check(const char* who, const void* fbank, const void* sbank, const void* workspace, const int* desc, int nslots, int nactive,
                     int max_nkeys, int Tcap, int H, int W, int C, int COcap, int topk) {
  if (H < 1 || W < 1 || C < 1 || COcap < 1 || COcap > LP_MAX_CLASSES || Tcap < 1) return fail(VFS_ERR_SHAPE, who, "H, W, C, Tcap >= 1, 1 <= COcap <= 256");
  if (nslots < 1 || nslots > LPB_MAX_SLOTS || nactive < 0 || nactive > nslots) return fail(VFS_ERR_SHAPE, who, "1 <= nslots <= 64, 0 <= nactive <= nslots");
  if (max_nkeys < 1 || max_nkeys > LP_MAX_KEYS) return fail(VFS_ERR_SHAPE, who, "1 <= max_nkeys <= 64");
  if (topk < 1 || topk > 10) return fail(VFS_ERR_SHAPE, who, "1 <= topk <= 10");
  if (!fbank || !sbank || !workspace || !desc) return fail(VFS_ERR_ARG, who, "null buffer");
  return VFS_OK;
}
static LpBatchArgs lpb_args(const float* fbank, const vfs_bf16* hl, float* sbank, char* ws, long long ws_stride, int* flags, const int* desc,
                            int nslots, int max_nkeys, int Tcap, int H, int W, int C, int COcap, int radius, int topk, float temperature) {
  LpBatchArgs b{};
  b.fbank = fbank; b.hl = hl; b.sbank = sbank; b.ws = ws; b.ws_stride = ws_stride; b.flags = flags; b.desc = desc;
  b.nslots = nslots; b.max_nkeys = max_nkeys; b.Tcap = Tcap; b.H = H; b.W = W; b.C = C; b.COcap = COcap;
  b.radius = radius; b.topk = topk; b.temperature = temperature;
  return b;
}
int vfs_labelprop_f32_batch_workspace_bytes(int H, int W, int nslots, long long* bytes) {
  if (!bytes || H <= 0 || W <= 0 || nslots < 1 || nslots > LPB_MAX_SLOTS)
    return vfs_set_error(VFS_ERR_ARG, "labelprop_f32_batch_workspace_bytes: bad argument");
  *bytes = nslots * lpb_round(lp_workspace_need(H, W));
  return VFS_OK;
}
int vfs_labelprop_f32_batch(const float* fbank, float* sbank, void* workspace, long long workspace_bytes, const int* desc, int nslots,
                            int nactive, int max_nkeys, int Tcap, int H, int W, int C, int COcap, int radius, int topk, float temperature,
                            vfs_stream_t stream) {
  if (int rc = lpb_check("labelprop_f32_batch", fbank, sbank, workspace, desc, nslots, nactive, max_nkeys, Tcap, H, W, C, COcap, topk)) return rc;
  const long long stride = lpb_round(lp_workspace_need(H, W));
  if (workspace_bytes < nslots * stride)
    return vfs_set_error(VFS_ERR_ARG, "labelprop_f32_batch: workspace smaller than vfs_labelprop_f32_batch_workspace_bytes(H, W, nslots)");
  if (nactive == 0) return VFS_OK;
  const LpBatchArgs b = lpb_args(fbank, nullptr, sbank, (char*)workspace, stride, nullptr, desc, nslots, max_nkeys, Tcap, H, W, C, COcap, radius,
                                 topk, temperature);
  return vfs_labelprop_f32_batch_launch(b, nactive, stream_of(stream));
}
int vfs_labelprop_f32_2pass_batch_workspace_bytes(int H, int W, int entries_per_query, int nslots, long long* bytes) {
  long long one = 0;
  if (!bytes || nslots < 1 || nslots > LPB_MAX_SLOTS ||
      vfs_labelprop_f32_2pass_workspace_bytes_for(H, W, entries_per_query > 0 ? entries_per_query : LP2_MAX_SPLIT * LP2_MAX_CAP, &one) != VFS_OK)
    return vfs_set_error(VFS_ERR_ARG, "labelprop_f32_2pass_batch_workspace_bytes: bad argument (0 or at least 16 list entries per query, 1 <= nslots <= 64)");
  *bytes = LPB_FLAG_BYTES + nslots * lpb_round(one);
  return VFS_OK;
}
int vfs_labelprop_f32_2pass_batch(const float* fbank, const vfs_bf16* hlbank, float* sbank, void* workspace, long long workspace_bytes,
                                  const int* desc, int nslots, int nactive, int max_nkeys, int Tcap, int H, int W, int C, int COcap, int radius,
                                  int topk, float temperature, int unit_rows, vfs_stream_t stream) {
  if (int rc = lpb_check("labelprop_f32_2pass_batch", fbank, sbank, workspace, desc, nslots, nactive, max_nkeys, Tcap, H, W, C, COcap, topk)) return rc;
  long long need = 0, dense = 0;
  if (vfs_labelprop_f32_2pass_batch_workspace_bytes(H, W, 16, nslots, &need) != VFS_OK || vfs_labelprop_workspace_bytes(H, W, &dense) != VFS_OK ||
      workspace_bytes < need)
    return vfs_set_error(VFS_ERR_ARG, "labelprop_f32_2pass_batch: workspace smaller than vfs_labelprop_f32_2pass_batch_workspace_bytes(H, W, 16, nslots)");
  if (nactive == 0) return VFS_OK;
  // [overflow words of the slots][slot 0: the single-video layout][slot 1] ...; the list capacity follows the bytes per slot
  const long long stride = (workspace_bytes - LPB_FLAG_BYTES) / nslots / 256 * 256;
  char* ws = (char*)workspace + LPB_FLAG_BYTES;
  LpBatchArgs b = lpb_args(fbank, hlbank, sbank, ws, stride, nullptr, desc, nslots, max_nkeys, Tcap, H, W, C, COcap, radius, topk, temperature);
  if (!hlbank || !unit_rows || !vfs_lp2_eligible(C) || (long long)H * W >= (1 << 21))      // as vfs_labelprop_f32_2pass: the dense kernels
    return vfs_labelprop_f32_batch_launch(b, nactive, stream_of(stream));
  const long long entries = (stride - dense - lp2_counts_bytes(H, W) - 16) / ((long long)H * W * 8);
  b.entries = (int)(entries > LP2_MAX_SPLIT * LP2_MAX_CAP ? LP2_MAX_SPLIT * LP2_MAX_CAP : entries);
  b.lists_bytes = lp2_lists_bytes(H, W, b.entries);
  b.flags = (int*)workspace;
  if (int rc = vfs_labelprop_f32_2pass_batch_launch(b, nactive, stream_of(stream))) return rc;
  // the dense kernels behind them: a slot whose lists overflowed is redone, the workgroups of the others leave at once
  return vfs_labelprop_f32_batch_launch(b, nactive, stream_of(stream));
}
// the bf16 kernels (labelprop.hip): the dense workspace per slot, the split of every slot as its single-video call chooses it
int vfs_labelprop_batch_workspace_bytes(int H, int W, int nslots, long long* bytes) {
  if (!bytes || H <= 0 || W <= 0 || nslots < 1 || nslots > LPB_MAX_SLOTS) return vfs_set_error(VFS_ERR_ARG, "labelprop_batch_workspace_bytes: bad argument");
  *bytes = nslots * lpb_round(lp_workspace_need(H, W));
  return VFS_OK;
}
int vfs_labelprop_batch(const vfs_bf16* fbank, float* sbank, void* workspace, long long workspace_bytes, const int* desc, int nslots, int nactive,
                        int max_nkeys, int Tcap, int H, int W, int C, int COcap, int radius, int topk, float temperature, vfs_stream_t stream) {
  if (int rc = lpb_check("labelprop_batch", fbank, sbank, workspace, desc, nslots, nactive, max_nkeys, Tcap, H, W, C, COcap, topk)) return rc;
  if (C % 64) return vfs_set_error(VFS_ERR_SHAPE, "labelprop_batch: C%64");
  if ((long long)H * W > 0x7fffffff / LP_MAX_KEYS) return vfs_set_error(VFS_ERR_SHAPE, "labelprop_batch: nkeys * H * W must fit the int candidate ids");
  if (!(temperature > 0.f)) return vfs_set_error(VFS_ERR_ARG, "labelprop_batch: temperature > 0");
  const long long stride = lpb_round(lp_workspace_need(H, W));
  if (workspace_bytes < nslots * stride)
    return vfs_set_error(VFS_ERR_ARG, "labelprop_batch: workspace smaller than vfs_labelprop_batch_workspace_bytes(H, W, nslots)");
  if (nactive == 0) return VFS_OK;
  LpBatchArgs b = lpb_args(nullptr, nullptr, sbank, (char*)workspace, stride, nullptr, desc, nslots, max_nkeys, Tcap, H, W, C, COcap, radius, topk,
                           temperature);
  b.fbank16 = fbank; b.inv_temp = 1.0f / temperature;
  return vfs_labelprop_batch_launch(b, stream_of(stream));
}
static int seg_post_batch_check(const char* who, const void* sbank, const void* partial, const void* preds, const int* desc, int nslots, int Tcap,
                                int Tmaps, int H, int W, int COcap, int Ho, int Wo) {
  if (H < 1 || W < 1 || Ho < 1 || Wo < 1 || COcap < 1 || COcap > LP_MAX_CLASSES || Tcap < 1 || Tmaps < 1 || nslots < 1 || nslots > LPB_MAX_SLOTS)
    return fail(VFS_ERR_SHAPE, who, "H, W, Ho, Wo, Tcap, Tmaps >= 1, 1 <= classes <= 256, 1 <= nslots <= 64");
  if ((long long)Ho * Wo > 0x7fffffff - 255 || (long long)H * W * COcap > 0x7fffffff)
    return fail(VFS_ERR_SHAPE, who, "Ho * Wo and H * W * classes must fit an int");
  if (!sbank || !partial || !preds || !desc) return fail(VFS_ERR_ARG, who, "null buffer");
  return VFS_OK;
}
int vfs_seg_postprocess_batch(const float* sbank, float* partial, uint8_t* preds, const int* desc, int nslots, int Tcap, int Tmaps, int H, int W,
                              int COcap, int Ho, int Wo, vfs_stream_t stream) {
  if (int rc = seg_post_batch_check("seg_postprocess_batch", sbank, partial, preds, desc, nslots, Tcap, Tmaps, H, W, COcap, Ho, Wo)) return rc;
  return vfs_seg_postprocess_batch_launch(sbank, partial, preds, desc, nslots, Tcap, Tmaps, H, W, COcap, Ho, Wo, stream_of(stream));
}
int vfs_seg_postprocess_exact_batch(const float* sbank, float* partial, uint8_t* preds, const int* desc, int nslots, int Tcap, int Tmaps, int H,
                                    int W, int COcap, int Ho, int Wo, vfs_stream_t stream) {
  if (int rc = seg_post_batch_check("seg_postprocess_exact_batch", sbank, partial, preds, desc, nslots, Tcap, Tmaps, H, W, COcap, Ho, Wo)) return rc;
  return vfs_seg_postprocess_exact_batch_launch(sbank, partial, preds, desc, nslots, Tcap, Tmaps, H, W, COcap, Ho, Wo, stream_of(stream));
}
int vfs_bilinear_resize_f32_batch(const float* sbank, float* preds, const int* desc, int nslots, int Tcap, int Tmaps, int H, int W, int COcap,
                                  int Ho, int Wo, vfs_stream_t stream) {
  if (Tcap < 1 || Tmaps < 1 || nslots < 1 || nslots > LPB_MAX_SLOTS)
    return vfs_set_error(VFS_ERR_SHAPE, "bilinear_resize_f32_batch: Tcap, Tmaps >= 1, 1 <= nslots <= 64");
  if (!sbank || !preds || !desc) return vfs_set_error(VFS_ERR_ARG, "bilinear_resize_f32_batch: null buffer");
  return vfs_bilinear_resize_f32_batch_launch(sbank, preds, desc, nslots, Tcap, Tmaps, H, W, COcap, Ho, Wo, stream_of(stream));
}
int vfs_bilinear_resize_f32(const float* src, float* dst, int C, int H, int W, int Ho, int Wo, int src_nhwc, int dst_nhwc,
                            vfs_stream_t stream) {
  if (!src || !dst) return vfs_set_error(VFS_ERR_ARG, "bilinear_resize_f32: null buffer");
  return vfs_bilinear_resize_f32_launch(src, dst, C, H, W, Ho, Wo, src_nhwc, dst_nhwc, stream_of(stream));
}
int vfs_seg_postprocess_exact(const float* seg, float* partial, uint8_t* label, int H, int W, int CO, int Ho, int Wo,
                              vfs_stream_t stream) {
  return vfs_seg_postprocess_exact_launch(seg, partial, label, H, W, CO, Ho, Wo, stream_of(stream));
}
// ---- table-driven ingest of a feature bank (bank_ingest.hip): the checks both precisions share, and the argument struct ----
static int bank_ingest_args(const char* who, BankIngestArgs* a, const void* feats, void* fbank, vfs_bf16* hlbank, const long long* table, int n,
                            long long P, int C, long long bank_rows, int unit_rows) {
  if (n < 1 || n > BANK_INGEST_MAX_N) return fail(VFS_ERR_SHAPE, who, "1 <= n <= 65535 images");
  if (P < 1 || P > 4LL * 0x7fffffff || C < 1 || bank_rows < P) return fail(VFS_ERR_SHAPE, who, "P >= 1 (four rows per workgroup), C >= 1, bank_rows >= P");
  if (!feats || !fbank || !table) return fail(VFS_ERR_ARG, who, "null buffer");
  if (hlbank && !unit_rows) return fail(VFS_ERR_ARG, who, "a split copy is taken of unit rows only");
  if (((size_t)feats | (size_t)fbank | (size_t)hlbank) & 15 || (size_t)table & 7)
    return fail(VFS_ERR_SHAPE, who, "16-byte aligned feature maps and banks, 8-byte aligned table");
  *a = BankIngestArgs{};
  a->x = feats; a->fbank = fbank; a->hl = hlbank; a->table = table; a->P = P; a->bank_rows = bank_rows; a->n = n; a->C = C; a->unit = unit_rows != 0;
  return VFS_OK;
}
int vfs_bank_ingest_f32(const float* feats, float* fbank, vfs_bf16* hlbank, const long long* table, int n, long long P, int C,
                        long long bank_rows, int unit_rows, vfs_stream_t stream) {
  BankIngestArgs a;
  if (int rc = bank_ingest_args("bank_ingest_f32", &a, feats, fbank, hlbank, table, n, P, C, bank_rows, unit_rows)) return rc;
  return vfs_bank_ingest_f32_launch(a, stream_of(stream));
}
int vfs_bank_ingest_bf16(const vfs_bf16* feats, vfs_bf16* fbank, const long long* table, int n, long long P, int C, long long bank_rows,
                         int unit_rows, vfs_stream_t stream) {
  BankIngestArgs a;
  if (int rc = bank_ingest_args("bank_ingest_bf16", &a, feats, fbank, nullptr, table, n, P, C, bank_rows, unit_rows)) return rc;
  return vfs_bank_ingest_bf16_launch(a, stream_of(stream));
}

int vfs_davis_counts(const uint8_t* pred, const uint8_t* gt, int* counts, void* scratch, int T, int H, int W, int nobj, int radius,
                     int use_void, vfs_stream_t stream) {
  if (T >= 3 && nobj > 0 && (!pred || !gt || !counts || !scratch)) return vfs_set_error(VFS_ERR_ARG, "davis_counts: null buffer");
  DavisArgs a{};
  a.pred = pred; a.gt = gt; a.counts = counts;
  a.bp = (unsigned*)scratch;
  a.bg = scratch ? (unsigned*)scratch + (size_t)(T > 2 ? T - 2 : 0) * H * W : nullptr;
  a.T = T; a.H = H; a.W = W; a.nobj = nobj; a.radius = radius; a.use_void = use_void;
  return vfs_davis_counts_launch(a, stream_of(stream));
}

int vfs_heatmap_topk(const float* maps, float* vals, int* idx, float* minv, int* flags, long long N, int H, int W, int topk,
                     vfs_stream_t stream) {
  if (N > 0 && (!maps || !vals || !idx || !minv || !flags)) return vfs_set_error(VFS_ERR_ARG, "heatmap_topk: null buffer");
  if (((uintptr_t)maps & 3u) != 0) return vfs_set_error(VFS_ERR_ARG, "heatmap_topk: maps must be 4-byte aligned");
  if (H < 1 || W < 1 || (long long)H * W > (1LL << 28)) return vfs_set_error(VFS_ERR_SHAPE, "heatmap_topk: 1 <= H*W <= 2^28");
  HeatmapTopkArgs a{};
  a.maps = maps; a.vals = vals; a.idx = idx; a.minv = minv; a.flags = flags;
  a.N = N; a.HW = H * W; a.topk = topk;
  return vfs_heatmap_topk_launch(a, stream_of(stream));
}

int vfs_label_counts(const uint8_t* pred, const uint8_t* gt, unsigned long long* counts, long long n, int num_classes,
                     int ignore_index, vfs_stream_t stream) {
  if (n > 0 && (!pred || !gt || !counts)) return vfs_set_error(VFS_ERR_ARG, "label_counts: null buffer");
  if (((uintptr_t)counts & 7u) != 0) return vfs_set_error(VFS_ERR_ARG, "label_counts: counts must be 8-byte aligned");
  LabelCountsArgs a{};
  a.pred = pred; a.gt = gt; a.counts = counts;
  a.n = n; a.num_classes = num_classes; a.ignore_index = ignore_index;
  return vfs_label_counts_launch(a, stream_of(stream));
}

int vfs_pose_heatmaps(const float* patch, const int* kp, float* out, int K, int H, int W, int P, vfs_stream_t stream) {
  if (K > 0 && (!patch || !kp || !out)) return vfs_set_error(VFS_ERR_ARG, "pose_heatmaps: null buffer");
  PoseHeatmapArgs a{};
  a.patch = patch; a.kp = kp; a.out = out;
  a.K = K; a.H = H; a.W = W; a.P = P;
  return vfs_pose_heatmaps_launch(a, stream_of(stream));
}

int vfs_crop_resize_flip_norm(const uint8_t* src, const int* boxes, const uint8_t* flips, float* imgs, vfs_bf16* x4, int B, int V, int T,
                              int Hs, int Ws, int Ho, int Wo, int Wp, double mean_r, double mean_g, double mean_b, double std_r,
                              double std_g, double std_b, vfs_stream_t stream) {
  const PipelineArgs a = pipeline_args(src, boxes, flips, imgs, x4, B, V, T, Hs, Ws, Ho, Wo, Wp, mean_r, mean_g, mean_b, std_r, std_g, std_b);
  return pipeline_run("crop_resize_flip_norm", a, stream_of(stream));
}

int vfs_crop_resize_flip_photo_norm_workspace_bytes(int frames, int Ho, int Wo, long long* bytes) {
  if (!bytes || frames <= 0 || Ho <= 0 || Wo <= 0) return vfs_set_error(VFS_ERR_ARG, "crop_resize_flip_photo_norm_workspace_bytes: bad argument");
  *bytes = vfs_photo_workspace_bytes(frames, Ho, Wo);
  return VFS_OK;
}

int vfs_crop_resize_flip_photo_norm(const uint8_t* src, const int* boxes, const uint8_t* flips, const int* photo, void* workspace,
                                    long long workspace_bytes, float* imgs, vfs_bf16* x4, int B, int V, int T, int Hs, int Ws, int Ho,
                                    int Wo, int Wp, double mean_r, double mean_g, double mean_b, double std_r, double std_g,
                                    double std_b, vfs_stream_t stream) {
  const PipelineArgs a = pipeline_args(src, boxes, flips, imgs, x4, B, V, T, Hs, Ws, Ho, Wo, Wp, mean_r, mean_g, mean_b, std_r, std_g, std_b);
  return photo_run("crop_resize_flip_photo_norm", a, photo, workspace, workspace_bytes, 0, stream_of(stream));
}

int vfs_crop_resize_flip_photo_norm_blur(const uint8_t* src, const int* boxes, const uint8_t* flips, const int* photo, void* workspace,
                                         long long workspace_bytes, float* imgs, vfs_bf16* x4, int B, int V, int T, int Hs, int Ws, int Ho,
                                         int Wo, int Wp, double mean_r, double mean_g, double mean_b, double std_r, double std_g,
                                         double std_b, int max_blur_radius, vfs_stream_t stream) {
  const PipelineArgs a = pipeline_args(src, boxes, flips, imgs, x4, B, V, T, Hs, Ws, Ho, Wo, Wp, mean_r, mean_g, mean_b, std_r, std_g, std_b);
  return photo_run("crop_resize_flip_photo_norm_blur", a, photo, workspace, workspace_bytes, max_blur_radius, stream_of(stream));
}

int vfs_crop_resize_flip_norm_ragged(const uint8_t* src, long long src_bytes, const int* srcdesc, const int* boxes, const uint8_t* flips,
                                     float* imgs, vfs_bf16* x4, int B, int V, int T, int Ho, int Wo, int Wp, double mean_r, double mean_g,
                                     double mean_b, double std_r, double std_g, double std_b, vfs_stream_t stream) {
  const PipelineArgs a = ragged_args(pipeline_args(src, boxes, flips, imgs, x4, B, V, T, 0, 0, Ho, Wo, Wp, mean_r, mean_g, mean_b, std_r, std_g,
                                                   std_b), srcdesc, src_bytes);
  return pipeline_run("crop_resize_flip_norm_ragged", a, stream_of(stream));
}

int vfs_crop_resize_flip_photo_norm_ragged(const uint8_t* src, long long src_bytes, const int* srcdesc, const int* boxes,
                                           const uint8_t* flips, const int* photo, void* workspace, long long workspace_bytes, float* imgs,
                                           vfs_bf16* x4, int B, int V, int T, int Ho, int Wo, int Wp, double mean_r, double mean_g,
                                           double mean_b, double std_r, double std_g, double std_b, vfs_stream_t stream) {
  const PipelineArgs a = ragged_args(pipeline_args(src, boxes, flips, imgs, x4, B, V, T, 0, 0, Ho, Wo, Wp, mean_r, mean_g, mean_b, std_r, std_g,
                                                   std_b), srcdesc, src_bytes);
  return photo_run("crop_resize_flip_photo_norm_ragged", a, photo, workspace, workspace_bytes, 0, stream_of(stream));
}

int vfs_crop_resize_flip_photo_norm_blur_ragged(const uint8_t* src, long long src_bytes, const int* srcdesc, const int* boxes,
                                                const uint8_t* flips, const int* photo, void* workspace, long long workspace_bytes,
                                                float* imgs, vfs_bf16* x4, int B, int V, int T, int Ho, int Wo, int Wp, double mean_r,
                                                double mean_g, double mean_b, double std_r, double std_g, double std_b, int max_blur_radius,
                                                vfs_stream_t stream) {
  const PipelineArgs a = ragged_args(pipeline_args(src, boxes, flips, imgs, x4, B, V, T, 0, 0, Ho, Wo, Wp, mean_r, mean_g, mean_b, std_r, std_g,
                                                   std_b), srcdesc, src_bytes);
  return photo_run("crop_resize_flip_photo_norm_blur_ragged", a, photo, workspace, workspace_bytes, max_blur_radius, stream_of(stream));
}

}  // extern "C"
