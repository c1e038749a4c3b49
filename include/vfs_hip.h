/* libvfs_hip.so -- C ABI of the MI355X (gfx950) VFS hot path.
 *
 * The reference (xvjiarui/VFS) has no native code: every function below replaces a torch /
 * mmcv call site of its Python hot path (file:line under /root/reference cited per entry).
 * A maintainer of the reference binds these with ctypes underneath the
 * same registry classes (ResNet / SimSiamHead / CosineSimLoss / SimSiamBaseTracker /
 * VanillaTracker); vfs_amd/ is exactly that binding.
 *
 * Conventions
 *   - the caller owns every buffer (device pointers from its allocator); the library keeps no
 *     device state and never synchronises: all work is enqueued on `stream` (a hipStream_t)
 *   - activations: bf16 NHWC; packed weights: bf16 [Cout][KH][KW][Cin] (forward) and
 *     [Cin][KH][KW][Cout] (dgrad); master parameters / gradients: fp32 in the reference's
 *     layouts (OIHW conv, [out][in] linear) so state_dicts stay interchangeable
 *   - return 0 on success, negative on error; vfs_last_error() gives the message
 *   - thread-safe per stream; one process per GPU.  The operator entry points below read no mutable library state except the A/B
 *     switchboard of include/vfs_hip_tuning.h, which a production caller never touches (every knob defaults to the measured-best path)
 */
#ifndef VFS_HIP_H
#define VFS_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* vfs_stream_t; /* hipStream_t */
typedef uint16_t vfs_bf16;

const char* vfs_last_error(void);
int vfs_abi_version(void);
/* (Measurement knobs - vfs_set_option - are NOT part of this contract: include/vfs_hip_tuning.h.) */

/* ---- input / parameter layout -------------------------------------------------------------
 * imgs fp32 [B][2][3][T][H][W] (pipelines/formating.py:248-258) -> bf16 NHWC4 frames
 * out[(v*B+b)*T+t][h][w][4], i.e. video2images(imgs[:, v]) per view
 * (sim_siam_base_tracker.py:65-68, common/utils.py:45-53); width padded to even Wp with zeros */
int vfs_imgs_to_nhwc4(const float* imgs, vfs_bf16* out, int B, int V, int T, int H, int W, int Wp,
                      vfs_stream_t stream);

/* table-driven repack of ALL fp32 master weights into the bf16 MFMA layouts in one launch.
 * desc: device array of ntensors records {w, wf, wd, start, Cout, Cin, KH, KW, kind, tile_start}
 * (8-byte pointers/int64 then 6 int32; kind 1 = 7x7 stem -> [64][8][8][4]).  One workgroup per
 * 32x32 (cout x cin) tile of a tensor (per 256 elements of the stem); tile_start = running sum,
 * total_tiles = its end (KH*KW <= 25 except the stem).  kind 2 / 3 = kind 0 with 16-byte accesses for the shapes that hold a
 * ResNet's weights - 2: 1x1 with 64 | Cout, 64 | Cin (one workgroup per 64 x 64 tile), 3: 3x3 with 32 | Cout, 64 | Cin (per 32 x 64
 * tile); w, wf, wd 16-byte aligned; identical results (the table builder of vfs_amd/packing.py chooses them). */
int vfs_pack_weights(const void* desc, int ntensors, long long total_tiles, vfs_stream_t stream);

/* ---- convolution / linear: torch conv2d & linear call sites ---------------------------------
 * forward  (resnet.py:51-73,163-191,267-277 via mmcv ConvModule; sim_siam_head.py:78-111):
 *   y[N,Ho,Wo,Cout] = conv(x[N,H,W,Cin], wf) (+ bias)          Cin % 64 == 0, Cout % 64 == 0
 *   stats (optional): float[rows][2][Cout] per-128-pixel-block (sum, sumsq) of the
 *   stored bf16 outputs -- the BatchNorm batch statistics, free in the GEMM epilogue; rows = ceil(N*Ho*Wo/128) linear blocks, or
 *   the spatial tiles of the 3x3 halo kernel: vfs_conv_plan says which and how many */
int vfs_conv_fwd(const vfs_bf16* x, const vfs_bf16* wf, vfs_bf16* y, const float* bias, float* stats,
                 int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                 int pad, vfs_stream_t stream);
/* vfs_conv_fwd that ALSO sums its statistics rows in groups of 2^coarse_log2 consecutive rows (round 5): the last workgroup of a
 * group to arrive (device-scope ticket) adds the group's rows in row order (deterministic) into
 *   stats_coarse: float[ceil(rows / 2^coarse_log2)][2][Cout]          rows = what vfs_conv_fwd writes to `stats`
 * so that the consumer finishing the BatchNorm statistics in its prologue (vfs_bn_act_fin, at most 128 rows per group) can be
 * used for the large maps as well and the separate reduction launch between conv and BatchNorm (torch: the batch_norm op's own
 * statistics pass, resnet.py via mmcv ConvModule) disappears.  tickets: uint32 [ceil(rows / 2^L) * ceil(Cout / 64)], zero before
 * the first launch, left at zero.  `stats` is still written (the fine rows are the exchange medium). */
int vfs_conv_fwd_coarse(const vfs_bf16* x, const vfs_bf16* wf, vfs_bf16* y, const float* bias, float* stats, float* stats_coarse,
                        uint32_t* tickets, int coarse_log2, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW,
                        int stride, int pad, vfs_stream_t stream);
/* 7x7/2 stem conv (resnet.py:422-434) on NHWC4 input, wf = [64][8][8][4].  stats rows: one per
 * spatial tile of 8x16 output pixels, N*ceil(Ho/8)*ceil(Wo/16) rows of [2][64] (image-major); ceil(N*Ho*Wo/128) linear rows on
 * the implicit-GEMM fallback (vfs_stem_plan reports the count in force) */
int vfs_stem_fwd(const vfs_bf16* x4, const vfs_bf16* wf, vfs_bf16* y, float* stats, int N, int H,
                 int Wp, int Ho, int Wo, vfs_stream_t stream);
/* dgrad (autograd of the above): dx[N,H,W,Cin] = conv_transpose(dy[N,Ho,Wo,Cout], wd) (+ add) */
int vfs_conv_dgrad(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, int N,
                   int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                   int pad, vfs_stream_t stream);
/* the same input gradient, plus the BatchNorm-backward statistics of the unit whose OUTPUT this gradient
 * belongs to, from the epilogue (saves bn_bwd_reduce's pass over dx): bn_partial float[ceil(M/128)][2][Cin]
 * rows {sum g*mask, sum g*mask*xhat} per 128 output pixels, M = N*H*W; bn_x = that unit's raw conv output
 * [M][Cin], bn_y its activation for the ReLU mask (residual units) or NULL (bn_relu: mask recomputed
 * from bn_x), bnp float[G][4][Cin], bn_mpg pixels per group (multiple of 128).  stride 1 only.
 * Feed bn_partial to vfs_bn_bwd_sums_paramgrad / vfs_bn_reduce_partials with bpg = bn_mpg/128. */
int vfs_conv_dgrad_bn(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add,
                      const vfs_bf16* bn_x, const vfs_bf16* bn_y, const float* bnp, float* bn_partial,
                      int bn_mpg, int bn_relu, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH,
                      int KW, int stride, int pad, vfs_stream_t stream);
/* vfs_conv_dgrad / vfs_conv_dgrad_bn whose `add` operand is gated by the bit-packed ReLU mask of its own tensor (add_mask: the
 * mask_bits of vfs_bn_act_mask for the [N,H,W,Cin] block output; NULL = plain add; Cin % 64 == 0): dx = dgrad + add * (y > 0).
 * The identity branch of a residual block (resnet.py:105-111,224-230: out = relu(bn(x) + identity)) then adds the
 * block-output gradient itself; the masked copy g * (y > 0) that vfs_bn_bwd_apply can emit (gm) is never written or read. */
int vfs_conv_dgrad_maskadd(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, const uint8_t* add_mask,
                           int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                           vfs_stream_t stream);
int vfs_conv_dgrad_bn_maskadd(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, const uint8_t* add_mask,
                              const vfs_bf16* bn_x, const vfs_bf16* bn_y, const float* bnp, float* bn_partial,
                              int bn_mpg, int bn_relu, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH,
                              int KW, int stride, int pad, vfs_stream_t stream);
/* dgrad of a 1x1 / stride-2 / pad-0 convolution (the downsample branch of a stage entry, resnet.py:267-277) without the zero planes:
 * such a convolution reads only the pixels with even h and even w, so three quarters of its input gradient are exactly zero and the
 * rest is the pure GEMM dy[N*Ho*Wo, Cout] x wd over the quarter grid, Ho = ceil(H / 2), Wo = ceil(W / 2); wd = [Cin][1][1][Cout].
 *   compact = 0: dx and add are DENSE [N,H,W,Cin] tensors of which only the pixels (n, 2 ho, 2 wo) are read and written:
 *                dx = dgrad + add there, every other pixel of dx keeps what it holds.  With add == dx (the residual branch's
 *                gradient, completed in place) the result equals vfs_conv_dgrad(..., stride 2) with the same add, bit for bit
 *                where the launch lands in a kernel of the same summation order.
 *   compact = 1: dx and add are contiguous [N,Ho,Wo,Cin] tensors, dx = dgrad (+ add).
 * add may be NULL.  The launch runs on the kernels of a 1x1 / stride-1 dgrad of the same pixel count (vfs_conv_dgrad_ds_plan:
 * wide = 128-channel tiles, ring = the LDS-DMA ring); Cin % 8 == 0, Cout % 64 == 0.  No mask-gated add, no statistics rows. */
int vfs_conv_dgrad_ds(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, int compact, int N, int H, int W,
                      int Cin, int Ho, int Wo, int Cout, vfs_stream_t stream);
int vfs_conv_dgrad_ds_plan(int compact, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int* wide, int* ring);
/* Split-K variants for problems with few output pixels and a long reduction - the SimSiam head's Linear
 * layers (sim_siam_head.py:78-111: 2048x2048 on 64 rows fill 16 workgroups otherwise): the K loop is cut into
 * ksplit slices that run as separate workgroups; the last slice to finish adds the fp32 partial tiles in
 * slice order (deterministic) and runs the usual epilogue (bias, statistics rows).  ks_ws: float workspace,
 * 1024 + tiles * ksplit * 128 * BC floats with tiles = ceil(M/128) * ceil(Cout/BC) <= 1024, BC = 128 when
 * Cout % 128 == 0 else 64; its first 1024 words (tickets) must be zero before the first launch and are left
 * zero.  Stride-1 problems only for the dgrad; ksplit == 1 is the plain kernel. */
int vfs_conv_fwd_splitk(const vfs_bf16* x, const vfs_bf16* wf, vfs_bf16* y, const float* bias, float* stats,
                        float* ks_ws, int ksplit, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH,
                        int KW, int stride, int pad, vfs_stream_t stream);
int vfs_conv_dgrad_splitk(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, float* ks_ws,
                          int ksplit, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW,
                          int stride, int pad, vfs_stream_t stream);
/* forward conv with dilated taps (resnet.py:51-58,172-179: ConvModule(padding=dilation, dilation=dilation) of a ResNet built
 * with dilations != 1 - the frozen backbone of the SiamFC probe, projects/siamfc-pytorch/siamfc/default_config_base.py:40-49).
 * Its backward: vfs_conv_dgrad_dilated / vfs_conv_wgrad_dilated below.  Ho = (H + 2 pad - dilation (KH - 1) - 1) / stride + 1. */
int vfs_conv_fwd_dilated(const vfs_bf16* x, const vfs_bf16* wf, vfs_bf16* y, const float* bias, float* stats, int N,
                         int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                         int dilation, vfs_stream_t stream);
/* dgrad of vfs_conv_fwd_dilated (torch autograd of the same call sites, resnet.py:51-58,172-179: ConvModule(padding=dilation,
 * dilation=dilation) wrt its input - a dilated backbone that is fine-tuned, siamfc_tracker_base.py:131-144 with frozen_stages < 4):
 *   dx[N,H,W,Cin] = sum over taps (r, s) and Cout of dy[N,Ho,Wo,Cout] at ((h + pad - r dilation) / stride, (w + pad - s dilation) /
 *   stride) * wd  (+ add, gated by add_mask)
 * bf16 NHWC operands, wd in the dgrad packing [Cin][KH][KW][Cout], fp32 accumulation on MFMA, ONE bf16 rounding of the output.
 * add / add_mask as in vfs_conv_dgrad_maskadd: the residual gradient added before the rounding and the bit-packed ReLU mask of its
 * own tensor that gates it (the identity branch of a dilated BasicBlock); both may be NULL (add_mask needs add).  No fused
 * BatchNorm-backward statistics: the consumer runs vfs_bn_bwd_reduce.  Stride 1 is the tuned case (the cost of the undilated
 * implicit-GEMM dgrad); stride > 1 is correct but gathers over the strided gradient: taps that fall between the samples of dy
 * are multiplied as inserted zeros.  Cin % 64 == 0, Cout % 64 == 0, KH * KW <= 32, every tensor below 4 GiB (VFS_ERR_SHAPE);
 * dilation >= 1 and non-null dy, wd, dx (VFS_ERR_ARG). */
int vfs_conv_dgrad_dilated(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, const uint8_t* add_mask,
                           int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                           int dilation, vfs_stream_t stream);
/* wgrad of vfs_conv_fwd_dilated (autograd of the same call sites wrt the weight), with the split-K contract of vfs_conv_wgrad:
 * partial: float[nsplit][Cout][KH*KW*Cin] over linear pixel ranges of pix_per_split pixels (pix_per_split % 64 == 0,
 * nsplit * pix_per_split >= N*Ho*Wo; pixels past N*Ho*Wo contribute exactly zero), summed in split order and ACCUMULATED into
 * grad[Cout][Cin][KH][KW] (fp32, OIHW); grad == NULL: only the partials are written (vfs_wgrad_reduce_table reduces them later; every
 * plan is taken as offered).  Bit-identical from run to run.  Same shape rules and error codes as vfs_conv_dgrad_dilated. */
int vfs_conv_wgrad_dilated(const vfs_bf16* dy, const vfs_bf16* x, float* partial, float* grad, int N, int H, int W, int Cin,
                           int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int dilation, int nsplit,
                           int pix_per_split, vfs_stream_t stream);
/* conv-BN-ReLU -> conv without materialising the activation: x_raw is the RAW output of the producer unit,
 * in_bnp its float[G][4][Cin] {scale, shift, mean, invstd}, in_npg images per group; relu(x*scale+shift)
 * (rounded to bf16 exactly as vfs_bn_act) is applied while the operand is staged, padding stays zero.
 * 3x3 / stride 1 / pad 1 on halo-tile-eligible shapes, and (round 6: the conv2 -> conv3 edge of a bottleneck block,
 * resnet.py:221-230) 1x1 / stride 1 / pad 0 with Cin % 64 == 0 and groups of whole 128-pixel tiles (in_npg*H*W % 128 == 0);
 * VFS_ERR_SHAPE otherwise.  The matching weight gradient reads the same raw tensor.  Replaces vfs_bn_act + vfs_conv_fwd /
 * vfs_conv_wgrad. */
int vfs_conv_fwd_bnin(const vfs_bf16* x_raw, const float* in_bnp, int in_npg, const vfs_bf16* wf, vfs_bf16* y,
                      const float* bias, float* stats, int N, int H, int W, int Cin, int Ho, int Wo, int Cout,
                      int KH, int KW, int stride, int pad, vfs_stream_t stream);
int vfs_conv_wgrad_bnin(const vfs_bf16* dy, const vfs_bf16* x_raw, const float* in_bnp, int in_npg, float* partial,
                        float* grad, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW,
                        int stride, int pad, int nsplit, int pix_per_split, vfs_stream_t stream);
/* wgrad: grad[Cout][Cin][KH][KW] (fp32, reference OIHW layout) += sum_pixels dy * im2col(x).
 * partial: workspace float[nsplit][Cout][KH*KW*Cin]; pix_per_split % 64 == 0 and
 * nsplit*pix_per_split >= N*Ho*Wo.  Deterministic (fixed-order split-K reduction).
 * grad == NULL (here and in vfs_conv_wgrad_bnin / vfs_stem_wgrad / vfs_stem_wgrad_fused): only the partials are written;
 * the caller keeps `partial` alive and reduces many layers at once with vfs_wgrad_reduce_table. */
int vfs_conv_wgrad(const vfs_bf16* dy, const vfs_bf16* x, float* partial, float* grad, int N, int H,
                   int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                   int nsplit, int pix_per_split, vfs_stream_t stream);
int vfs_stem_wgrad(const vfs_bf16* dy, const vfs_bf16* x4, float* partial, float* grad, int N, int H,
                   int Wp, int Ho, int Wo, int nsplit, int pix_per_split, vfs_stream_t stream);
/* Round 6 - vfs_conv_wgrad / vfs_conv_wgrad_bnin with the split-K reduction INSIDE the launch (one launch per layer instead of
 * two): the last workgroup of a (k-column, cout) tile to arrive - a device-scope ticket per tile - adds the tile's partials in
 * ascending split order (run-to-run bit-identical, whichever workgroup arrives last) into grad.  Same operands as vfs_conv_wgrad
 * (torch autograd of F.conv2d / F.linear wrt the weight, resnet.py:163-191,221-230; sim_siam_head.py:78-111); in_bnp / in_npg as in
 * vfs_conv_wgrad_bnin or NULL / 0; grad must be given.  partial: workspace of nsplit * Cout * roundup(KH*KW*Cin, 128) floats (the
 * launch's own layout: whole 128-byte lines per wave, written and read back with device-scope accesses; its contents mean nothing
 * to the caller).  tickets: unsigned[vfs_wgrad_tickets()] in device memory, ZERO before the
 * first launch; every launch leaves it zero, so one array serves all launches of a stream (launches that may overlap on different
 * streams need their own).  Gradients equal the two-launch form's up to the fp32 summation order of the splits. */
int vfs_wgrad_tickets(void);
int vfs_conv_wgrad_inl(const vfs_bf16* dy, const vfs_bf16* x, const float* in_bnp, int in_npg, float* partial, float* grad,
                       unsigned* tickets, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                       int pad, int nsplit, int pix_per_split, vfs_stream_t stream);
/* db[Cout] += column sums of dy[M][Cout] (linear bias gradient) */
int vfs_bias_grad(const vfs_bf16* dy, float* db, int M, int C, vfs_stream_t stream);

/* ---- tiling plan queries (host only: nothing is launched) -----------------------------------------------------------------
 * The library alone decides which kernel family a convolution launch lands in and how its statistics rows are laid out; a host
 * that sizes the row buffers, tells the BatchNorm passes how many rows to sum, or splits a weight gradient asks here.  The
 * answers hold for the options in force (include/vfs_hip_tuning.h) at the time of the call and are what the entry points above do
 * with the same geometry: each query builds the launch's arguments and asks the dispatcher's own predicate.  All geometry
 * arguments are those of the FORWARD convolution, as in the entry points.  VFS_ERR_ARG on a null out-pointer, G < 1 or
 * dilation < 1.
 *
 * vfs_conv_plan: dgrad = 0 - vfs_conv_fwd / _coarse / _dilated / _bnin writing `stats` rows [2][Cout] for y[N,Ho,Wo,Cout];
 *                dgrad = 1 - vfs_conv_dgrad* (stride 1 or 2), vfs_conv_dgrad_bn* writing `bn_partial` rows [2][Cin] for dx[N,H,W,Cin].
 *   halo : 1 when the 3x3 halo-tile kernel takes the launch (rows are spatial tiles, image-major), 0: implicit-GEMM family
 *          (rows are linear 128-pixel blocks of the output)
 *   rows : statistics rows PER GROUP that ONE launch over all N images writes, when the N images form G BatchNorm groups of
 *          N / G consecutive images (the buffer holds G * rows rows, group after group); 0: a group does not own whole rows -
 *          launch once per group (N / G images, G = 1).  Always 0 for a stride-2 dgrad, which writes no rows.
 *   pairs: 1 when the halo kernels of this layer tile whole images of at most 8x8 pixels in PAIRS: vfs_conv_fwd_bnin /
 *          vfs_conv_wgrad_bnin then need an even in_npg.
 * vfs_stem_plan: rows per group (as above) that vfs_stem_fwd writes - one per 8x16 output tile with the direct kernel, one per
 *   128 output pixels when it falls back to the implicit-GEMM kernel (option stem_direct = 0, inputs of 4 GiB and more).
 * vfs_conv_wgrad_plan: halo = 1 when vfs_conv_wgrad / _bnin / _inl run the 3x3 halo kernel; ntiles = the spatial tiles that
 *   kernel splits over (it takes min(nsplit, ntiles) splits of ceil(ntiles / nsplit) tiles), 0 when halo = 0 (the generic kernel
 *   splits over linear pixel ranges of pix_per_split pixels). */
int vfs_conv_plan(int dgrad, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                  int dilation, int G, int* halo, int* rows, int* pairs);
int vfs_stem_plan(int N, int H, int Wp, int Ho, int Wo, int G, int* rows);
int vfs_conv_wgrad_plan(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int* halo,
                        int* ntiles);

/* ---- BatchNorm / SyncBN + activation (torch batch_norm in ConvModule; configs/r*_*.py:9,15) ------
 * G = number of independent BN batches inside the tensor (the two views), bpg partial blocks
 * per group.  sums: double[G][2][C]; between reduce_partials and finalize the host all-reduces
 * `sums` across ranks for SyncBN (count = global element count per channel per group).
 * bnp: float[G][4][C] = {scale, shift, mean, invstd}. */
int vfs_bn_reduce_partials(const float* partial, double* sums, double* scratch, int G, int bpg, int C,
                           vfs_stream_t stream);
/* scratch (or NULL): 64 uint32 ticket counters, zero before the first use and left at zero by every
 * call, followed by double[G][128][2][C].  With it, large row counts are reduced by many workgroups
 * in ONE launch (the workgroup that draws the last ticket of a 32-channel block finishes it). */
int vfs_bn_finalize(const double* sums, const float* gamma, const float* beta, float* bnp,
                    float* running_mean, float* running_var, int G, int C, double count, float eps,
                    float momentum, vfs_stream_t stream);
/* vfs_bn_stats_finalize + vfs_bn_act in ONE launch, resp. vfs_bn_bwd_sums_paramgrad + vfs_bn_bwd_apply, for SMALL
 * statistics row counts (bpg <= ~128 rows per group: ResNet-50's 16x16 / 8x8 stages): every workgroup of the apply
 * pass reduces the partial rows of its own (group, <= 64-channel slab) in its prologue - same order everywhere, so the
 * coefficients are identical - and the first workgroup of a slab writes bnp / sums / running statistics (forward) or
 * sums / dgamma / dbeta (backward).  Removes a dependent ~6 us launch per BatchNorm layer and direction.
 * vfs_bn_act_fin with partial == NULL (SyncBN): `sums` already holds the all-reduced totals and count the global element
 * count; the kernel then replaces vfs_bn_finalize + vfs_bn_act for any tensor size. */
int vfs_bn_act_fin(const vfs_bf16* x, const float* partial, int bpg, const float* gamma, const float* beta, float* bnp,
                   double* sums, float* running_mean, float* running_var, const vfs_bf16* res, const vfs_bf16* rres,
                   const float* rbnp, vfs_bf16* y, long long M, int C, int mpg, int relu, double count, float eps,
                   float momentum, vfs_stream_t stream);
int vfs_bn_bwd_apply_fin(const vfs_bf16* g, const vfs_bf16* y, const vfs_bf16* x, const float* bnp, const float* partial,
                         int bpg, double* sums, float* dgamma, float* dbeta, vfs_bf16* dx, vfs_bf16* gm, long long M, int C,
                         int mpg, double count, int relu, vfs_stream_t stream);
/* the same result as vfs_bn_stats_finalize, computed from the stored bf16 output raw [G*rows_per_group][C] instead of the conv
 * kernels' 128-pixel statistics rows: for SMALL groups that are not multiples of 128 rows (the head's BN1d layers,
 * sim_siam_head.py:78-111, 32 rows per view on the ResNet-50 config), so that ONE conv launch covers all groups */
/* Round 6 - nn.Linear + BatchNorm1d (training statistics) + [ReLU] of the SimSiam head in ONE launch (sim_siam_head.py:78-111: the
 * projector / predictor units Linear -> BN -> ReLU on M = G * mpg <= 256 rows, G <= 4 views, K % 128 == 0, C % 16 == 0):
 * raw = x wf^T + bias (bf16, kept for the backward), statistics of the stored values per view, act = [relu](raw * scale + shift),
 * bnp / sums / running statistics as vfs_bn_stats_raw_finalize writes them - for <= 128 rows (where vfs_conv_fwd runs the skinny GEMM)
 * the same bits as vfs_conv_fwd + vfs_bn_stats_raw_finalize + vfs_bn_act, above that equal up to the K order of the GEMM; two
 * dependent launches less per unit.  Single-GPU path (SyncBN keeps the exchange). */
int vfs_linear_bn_act(const vfs_bf16* x, const vfs_bf16* wf, const float* bias, const float* gamma, const float* beta,
                      vfs_bf16* raw, vfs_bf16* act, float* bnp, double* sums, float* running_mean, float* running_var, int M,
                      int K, int C, int mpg, int relu, double count, float eps, float momentum, vfs_stream_t stream);
/* Round 6 - vfs_bn_bwd_reduce + vfs_bn_bwd_apply_fin in ONE launch for groups with a single statistics row (mpg | 512, or mpg < 16:
 * the BatchNorm1d layers of the SimSiam head, sim_siam_head.py:78-111, and tiny maps): the apply pass computes the row {sum g*mask,
 * sum g*mask*xhat} from (g, x, mask) in its prologue in vfs_bn_bwd_reduce's summation order - the same bits - and writes sums,
 * dgamma, dbeta, dx (gm) as vfs_bn_bwd_apply_fin does.  torch autograd of batch_norm (+ relu) on a [M][C] tensor. */
int vfs_bn_bwd_apply_raw(const vfs_bf16* g, const vfs_bf16* y, const vfs_bf16* x, const float* bnp, double* sums, float* dgamma,
                         float* dbeta, vfs_bf16* dx, vfs_bf16* gm, long long M, int C, int mpg, double count, int relu,
                         vfs_stream_t stream);
int vfs_bn_stats_raw_finalize(const vfs_bf16* raw, double* sums, const float* gamma, const float* beta, float* bnp,
                              float* running_mean, float* running_var, int G, int rows_per_group, int C, double count,
                              float eps, float momentum, vfs_stream_t stream);
/* single-process fast paths (no SyncBN all-reduce in between): vfs_bn_reduce_partials fused with
 * vfs_bn_finalize, resp. with vfs_bn_param_grad (sums are still written for the apply pass) */
int vfs_bn_stats_finalize(const float* partial, double* sums, double* scratch, const float* gamma,
                          const float* beta, float* bnp, float* running_mean, float* running_var, int G,
                          int bpg, int C, double count, float eps, float momentum, vfs_stream_t stream);
int vfs_bn_bwd_sums_paramgrad(const float* partial, double* sums, double* scratch, float* dgamma,
                              float* dbeta, int G, int bpg, int C, vfs_stream_t stream);
int vfs_bn_eval_params(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float* bnp, int C, float eps, vfs_stream_t stream);
/* y = [relu](x*scale+shift [+res] [+ rres*rscale+rshift])   (resnet.py:102-111,221-230) */
int vfs_bn_act(const vfs_bf16* x, const float* bnp, const vfs_bf16* res, const vfs_bf16* rres,
               const float* rbnp, vfs_bf16* y, long long M, int C, int mpg, int relu,
               vfs_stream_t stream);
/* vfs_bn_act / vfs_bn_act_fin with a second output: mask_bits, M*C/8 bytes, bit i of the byte of (pixel m, channels c..c+7) =
 * (y[m][c+i] > 0); bytes are stored SLAB-major, uint8 [C/64][M][8] ([M][C/8] when C < 64), so that a kernel that owns <= 64
 * channels of a pixel range reads contiguous bytes.
 * The BatchNorm backward of a residual unit (resnet.py:102-111,221-230: out = relu(bn(x) + identity)) needs y only as
 * that mask, in two passes (statistics, apply): pass the mask as `y` with relu = 2 to vfs_bn_bwd_reduce / vfs_bn_bwd_apply /
 * vfs_bn_bwd_apply_fin / vfs_conv_dgrad_bn (bn_relu = 2) and they read 1/16 of the bytes - bit-identical gradients. */
int vfs_bn_act_mask(const vfs_bf16* x, const float* bnp, const vfs_bf16* res, const vfs_bf16* rres,
                    const float* rbnp, vfs_bf16* y, uint8_t* mask_bits, long long M, int C, int mpg, int relu,
                    vfs_stream_t stream);
int vfs_bn_act_fin_mask(const vfs_bf16* x, const float* partial, int bpg, const float* gamma, const float* beta, float* bnp,
                        double* sums, float* running_mean, float* running_var, const vfs_bf16* res, const vfs_bf16* rres,
                        const float* rbnp, vfs_bf16* y, uint8_t* mask_bits, long long M, int C, int mpg, int relu,
                        double count, float eps, float momentum, vfs_stream_t stream);
/* stem: y = maxpool3x3/2/1(relu(bn(x)))  (resnet.py:435), idx = argmax code per element (tap 0..8 of the 3x3 window; 0xFF where
 * the pooled activation is not positive - no gradient flows there, and the kernels that route the gradient by the code
 * (vfs_maxpool_relu_bwd, vfs_stem_pool_bn_bwd_reduce with xpool, vfs_stem_pool_bn_bwd_apply, vfs_stem_wgrad_fused) take the ReLU mask
 * from it: their yp argument is kept for the signature, they do not read it); xpool (optional) = the RAW x at each argmax: the BatchNorm backward of the stem then
 * never re-reads x */
int vfs_bn_relu_maxpool(const vfs_bf16* x, const float* bnp, vfs_bf16* y, uint8_t* idx, vfs_bf16* xpool,
                        int N, int H, int W, int C, int Hp, int Wp, int npg, vfs_stream_t stream);
int vfs_maxpool_relu_bwd(const vfs_bf16* gp, const vfs_bf16* yp, const uint8_t* idx, vfs_bf16* ga,
                         int N, int H, int W, int C, int Hp, int Wp, vfs_stream_t stream);
/* BN backward: pass 1 -> partial[nblk][2][C] (S1 = sum gm, S2 = sum gm*xhat, gm = g*mask);
 * then vfs_bn_reduce_partials -> sums (all-reduce for SyncBN) -> pass 2.
 * mask: y != NULL -> (y > 0) (residual units); y == NULL && relu -> (x*scale+shift > 0); else 1 */
int vfs_bn_bwd_reduce(const vfs_bf16* g, const vfs_bf16* y, const vfs_bf16* x, const float* bnp,
                      float* partial, long long M, int C, int mpg, int ppb, int relu,
                      vfs_stream_t stream);
int vfs_bn_bwd_apply(const vfs_bf16* g, const vfs_bf16* y, const vfs_bf16* x, const float* bnp,
                     const double* sums, vfs_bf16* dx, vfs_bf16* gm, long long M, int C, int mpg,
                     double count, int relu, vfs_stream_t stream);
int vfs_bn_param_grad(const double* sums, float* dgamma, float* dbeta, int G, int C,
                      vfs_stream_t stream);
/* stem: BN backward through max-pool + ReLU without materialising the full-resolution gradient
 * (same results as vfs_maxpool_relu_bwd followed by vfs_bn_bwd_reduce / vfs_bn_bwd_apply);
 * pass 1 -> partial[ceil(N*Hp*Wp/ppb)][2][C], pass 2 -> dx[N][H][W][C] */
int vfs_stem_pool_bn_bwd_reduce(const vfs_bf16* gp, const vfs_bf16* yp, const uint8_t* idx,
                                const vfs_bf16* x, const vfs_bf16* xpool, const float* bnp, float* partial,
                                int N, int H, int W, int C, int Hp, int Wp, int npg, int ppb,
                                vfs_stream_t stream); /* xpool (from vfs_bn_relu_maxpool) replaces the gather from x */
/* stem weight gradient with the BN-backward apply pass folded into its operand load (the
 * full-resolution dx is never materialised): grad[64][3][7][7] += ...; partial: float[nblocks][64][224],
 * nblocks = ceil(ntiles / ceil(ntiles / nblocks)) with ntiles = N*ceil(Ho/8)*ceil(Wo/16) */
int vfs_stem_wgrad_fused(const vfs_bf16* x4, const vfs_bf16* xraw, const vfs_bf16* gp, const vfs_bf16* yp,
                         const uint8_t* idx, const float* bnp, const double* sums, float* partial,
                         float* grad, int N, int Hin, int Win, int Ho, int Wo, int Hp, int Wp, int npg,
                         double count, int nblocks, vfs_stream_t stream);
int vfs_stem_pool_bn_bwd_apply(const vfs_bf16* gp, const vfs_bf16* yp, const uint8_t* idx,
                               const vfs_bf16* x, const float* bnp, const double* sums, vfs_bf16* dx,
                               int N, int H, int W, int C, int Hp, int Wp, int npg, double count,
                               vfs_stream_t stream);

/* ---- head: AdaptiveAvgPool2d((1,1)) + flatten (sim_siam_head.py:117,154-157) ---------------- */
int vfs_avgpool_fwd(const vfs_bf16* x, vfs_bf16* y, int N, int HW, int C, vfs_stream_t stream);
int vfs_avgpool_bwd(const vfs_bf16* g, vfs_bf16* gx, int N, int HW, int C, vfs_stream_t stream);

/* ---- fp32 NCHW <-> bf16 NHWC: the boundary of the module-level autograd entry points (ResNet.forward, SimSiamHead.forward,
 * DenseSimSiamHead.forward in train mode) and the gradient joins of ResNet.backward_nhwc / SimSiamHead.backward_nhwc.
 * LDS-tiled transposes over [N][HW][C] <-> [N][C][HW]; HW is free, C a multiple of 64.  VFS_ERR_SHAPE for a null buffer, a
 * non-positive size, C % 64 != 0, or 2^31 and more 64 x 64 tiles; the NHWC buffers are 16-byte aligned (VFS_ERR_ARG).
 * vfs_nhwc_bf16_to_nchw_f32: dst = src.float().permute(0, 3, 1, 2).contiguous() of a stage output [N, h, w, C] (exact).
 * vfs_nchw_f32_to_nhwc_bf16: dst = g.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16) of a cotangent [N, C, h, w]: round to
 *   nearest even; Inf stays Inf, NaN stays NaN.
 * vfs_nchw_f32_add_nhwc_bf16: the join, dst = bf16_rne(acc.float() + src.permute(0, 2, 3, 1)) - ONE rounding of the fp32 sum, not
 *   the two of (acc + src.to(bf16)).  dst may be acc.
 * vfs_bf16_add: dst = (a.float() + b.float()).to(torch.bfloat16) over n elements (n % 8 == 0, n <= 2^40): the join of two bf16
 *   gradients in one launch.  dst may be a or b. */
int vfs_nhwc_bf16_to_nchw_f32(const vfs_bf16* src, float* dst, int N, int HW, int C, vfs_stream_t stream);
int vfs_nchw_f32_to_nhwc_bf16(const float* src, vfs_bf16* dst, int N, int HW, int C, vfs_stream_t stream);
int vfs_nchw_f32_add_nhwc_bf16(const float* src, const vfs_bf16* acc, vfs_bf16* dst, int N, int HW, int C, vfs_stream_t stream);
int vfs_bf16_add(const vfs_bf16* a, const vfs_bf16* b, vfs_bf16* dst, long long n, vfs_stream_t stream);

/* ---- CosineSimLoss over all temporal rolls (sim_loss.py:42-63, sim_siam_head.py:165-174,
 * sim_siam_base_tracker.py:31-56).  loss/gloss: float[K][N]; K = T (intra_video) or 1 */
int vfs_cosine_loss_fwd(const vfs_bf16* p1, const vfs_bf16* z1, const vfs_bf16* p2,
                        const vfs_bf16* z2, float* loss, int N, int C, int T, int K, int negative,
                        float weight, vfs_stream_t stream);
/* BaseTracker._parse_losses (trackers/base.py:76-110) of the K loss rows: means[k] = mean(loss[k][:]) for k < K,
 * means[K] = sum of the K means (the 'loss' entry); double accumulation, fixed order.  means: float[K+1] */
int vfs_loss_means(const float* loss, float* means, int K, int N, vfs_stream_t stream);
int vfs_cosine_loss_bwd(const vfs_bf16* p1, const vfs_bf16* z1, const vfs_bf16* p2,
                        const vfs_bf16* z2, const float* gloss, vfs_bf16* dp1, vfs_bf16* dp2, int N,
                        int C, int T, int K, int negative, float weight, vfs_stream_t stream);

/* ---- DenseSimSiamHead.loss over all temporal rolls (sim_siam_head.py:277-284: CosineSimLoss(with_norm=True, pairwise=False)
 * on 4-D operands, sim_loss.py:43-62, inside the roll loop of sim_siam_base_tracker.py:39-55), on the head's own bf16 NHWC
 * output: p1, z1, p2, z2 = [N][S][C], N = B*T images of one view, S = h*w positions, 16-byte aligned.
 *   loss[k][i] = weight * (0.5 * L(p1[i], z2[j]) + 0.5 * L(p2[j], z1[i])),  j = roll_k(i) within i's video of T frames,
 *   L(a, b) = negative ? -m : 2 - 2 m,  m = mean over the S positions of <a[s], b[s]> / (max(|a[s]|, 1e-12) max(|b[s]|, 1e-12)).
 *   bwd: dp1, dp2 [N][S][C] = gradient wrt p (z is detached), summed over the K rolls with gloss[K][N].
 * N % T == 0, 1 <= K <= T, S >= 1, C % 8 == 0, C <= 2048 (the backward keeps a position's operands and gradient in registers:
 * 4 16-byte chunks per lane at most).  No atomics: equal inputs give equal bits.  workspace: per-workgroup partial sums of the
 * forward, at least vfs_dense_cosine_loss_workspace_bytes(N, S, C, K) bytes (host-only query); a smaller buffer is REFUSED. */
int vfs_dense_cosine_loss_workspace_bytes(int N, int S, int C, int K, long long* bytes);
int vfs_dense_cosine_loss_fwd(const vfs_bf16* p1, const vfs_bf16* z1, const vfs_bf16* p2, const vfs_bf16* z2, float* loss,
                              void* workspace, long long workspace_bytes, int N, int S, int C, int T, int K, int negative,
                              float weight, vfs_stream_t stream);
int vfs_dense_cosine_loss_bwd(const vfs_bf16* p1, const vfs_bf16* z1, const vfs_bf16* p2, const vfs_bf16* z2,
                              const float* gloss, vfs_bf16* dp1, vfs_bf16* dp2, int N, int S, int C, int T, int K,
                              int negative, float weight, vfs_stream_t stream);

/* ---- CosineSimLoss on spatial inputs, incl. pairwise=True / mask / with_norm=False (sim_loss.py:42-63) -------------
 * fp32 [B][C][S] operands = the reference's [B,C,*] tensors flattened (`.flatten(2)`); Sa / Sl: positions of cls_score / label.
 * colnorm: inv[b][s] = 1 / max(||x[b][:][s]||_2, 1e-12)   (F.normalize(p=2, dim=1), :44-45); pass inv = NULL for with_norm=False.
 * fwd: pairwise = 1: prod = einsum('bci,bcj->bij') on the matrix cores (fp32 MFMA), * mask[B][Sa][Sl] when given, mean over
 *      (i, j) (:48-56); pairwise = 0 (Sa == Sl): sum over C per position, mean over positions (:57-58);
 *      loss[b] = weight * (negative ? -mean : 2 - 2 * mean) (:59-62, losses/base.py:37).  partial: float scratch
 *      [B][ceil(Sa/32) * ceil(Sl/32)].
 * bwd: d[B][C][Sself] = gradient wrt the NORMALISED operand of one side given gloss[B]; `other` is the opposite operand
 *      (raw) with its inverse norms; mask_transposed = 1 when this side is the einsum's j operand (label).
 * norm_bwd: dx = (d - x^ <x^, d>) * inv per position (backward of F.normalize); inv = NULL: dx = d. */
int vfs_simloss_colnorm(const float* x, float* inv, int B, int C, int S, vfs_stream_t stream);
int vfs_simloss_fwd(const float* a, const float* l, const float* inva, const float* invl, const float* mask,
                    float* partial, float* loss, int B, int C, int Sa, int Sl, int pairwise, int negative,
                    float weight, vfs_stream_t stream);
int vfs_simloss_bwd(const float* other, const float* invo, const float* mask, int mask_transposed,
                    const float* gloss, float* d, int B, int C, int Sself, int Sother, int pairwise,
                    int negative, float weight, vfs_stream_t stream);
int vfs_simloss_norm_bwd(const float* x, const float* inv, const float* d, float* dx, int B, int C, int S,
                         vfs_stream_t stream);

/* ---- Differentiable masked_attention (mmaction/models/common/local_attention.py:161-234 with the circular window of
 * spatial_neighbor, affinity_utils.py:144-156): forward, and backward wrt query, key and value ------------------------------
 * fp32 NCHW operands: query [N][C][H*W], key [N][C][T*H*W], value [N][CO][T*H*W], out / dout [N][CO][H*W].
 * score(i, j) = <k^_i, q^_j> / temperature over the keys i = (t, y', x') with (y - y')^2 + (x - x')^2 < (neighbor_range / 2)^2
 * of query j = (y, x) (the same window in every key frame; neighbor_range = 0: every key); k^, q^ = F.normalize(dim=1,
 * eps 1e-12) when normalize, the rows themselves otherwise (:194-196).  The topk largest (equal scores: the lower flat key
 * index first) are softmaxed and weight the value columns (:212-226).  The window is a test in the kernel: no mask, no
 * [T*H*W][H*W] affinity.
 *   fwd: writes out and what the backward needs: idx int32 [N][topk][H*W] (flat key index over T*H*W; -1 = the weight-0 fill
 *        of a query with fewer than topk in-window keys), weights fp32 [N][topk][H*W] (the softmax; 0 at a fill), and with
 *        normalize invq [N][H*W], invk [N][T*H*W] = 1 / max(||row||_2, 1e-12) (NULL allowed otherwise).
 *   bwd: ds_a = w_a (<v_a, dout_j> - sum_b w_b <v_b, dout_j>) / temperature;  dq^_j = sum_a ds_a k^_a;  dk^_i = sum over
 *        the (j, a) that selected i of ds_a q^_j;  dv_i = sum over the same of w_a dout_j;  dq, dk go through the
 *        normalisation (d x = inv (g - x^ <x^, g>), as vfs_simloss_norm_bwd).  dq / dk / dv = NULL: that gradient is not
 *        computed.  No atomics: each key scans the queries that can reach it in ascending index, equal inputs give equal bits.
 *        workspace: at least vfs_masked_attention_workspace_bytes(...) bytes (host-only query; the size for all three
 *        gradients); a smaller buffer is REFUSED (VFS_ERR_ARG).
 * VFS_ERR_SHAPE: topk outside 1..10, neighbor_range 1 or negative, C % 64 != 0 or C > 2048, T outside 1..64, CO outside
 * 1..256, T*H*W >= 2^31, N outside 1..65535.  VFS_ERR_ARG: a null operand, temperature not positive and finite. */
int vfs_masked_attention_workspace_bytes(int N, int C, int T, int H, int W, int CO, int topk, int normalize, long long* bytes);
int vfs_masked_attention_fwd(const float* query, const float* key, const float* value, float* out, int* idx, float* weights,
                             float* invq, float* invk, int N, int C, int T, int H, int W, int CO, int neighbor_range, int topk,
                             float temperature, int normalize, vfs_stream_t stream);
int vfs_masked_attention_bwd(const float* query, const float* key, const float* value, const float* dout, const int* idx,
                             const float* weights, const float* invq, const float* invk, float* dq, float* dk, float* dv,
                             void* workspace, long long workspace_bytes, int N, int C, int T, int H, int W, int CO,
                             int neighbor_range, int topk, float temperature, int normalize, vfs_stream_t stream);

/* ---- SyncBN statistic exchange over xGMI (configs/r*_*.py:9,15 SyncBN under MMDistributedDataParallel, apis/train.py:58-66):
 * a latency-bound all-reduce of <= 8192 doubles among the <= 8 ranks of one node as ONE small kernel - peer stores into
 * IPC-mapped windows + epoch flags (csrc/p2p.hip) - instead of a collective-library call per BatchNorm layer and direction.
 *   window_bytes: size of a window, the largest n and world supported
 *   alloc / free: a zeroed window in fine-grained device memory (hipExtMallocWithFlags)
 *   export: 64-byte IPC handle of the own window (hipIpcGetMemHandle); import / unimport: map / unmap a peer's window
 *   allreduce_f64: buf[0..n) <- sum over ranks, in rank order (bit-identical on every rank).  peers: DEVICE array of `world`
 *     window pointers (peers[rank] = the own window); state: 4 x uint64 in device memory, zero-initialised ({exchange
 *     counter, error flag, -, -}); phase 3 = push + wait (1 / 2: the halves, for protocol tests); spin_limit: polls before the
 *     kernel gives up, sets state[1] = 1 and returns garbage (a lost peer must not hang the GPU). */
int vfs_p2p_window_bytes(long long* bytes, int* max_doubles, int* max_world);
/* the SyncBN reductions with the exchange as their TAIL: vfs_bn_reduce_partials (forward: statistics rows -> sums) and
 * vfs_bn_bwd_sums_paramgrad (backward: rows -> sums + LOCAL dgamma / dbeta) whose last workgroup runs the window exchange on
 * sums[G][2][C] (G*2*C <= 8192) - no launch and no collective call between "local sums" and "sums over all ranks".
 * state: 4 x uint64, zero-initialised ({exchange counter, error flag, workgroup ticket, -}); other arguments as above. */
int vfs_bn_reduce_partials_xchg(const float* partial, double* sums, double* scratch, int G, int bpg, int C,
                                const void* peers, int rank, int world, void* state, long long spin_limit,
                                vfs_stream_t stream);
int vfs_bn_bwd_sums_paramgrad_xchg(const float* partial, double* sums, double* scratch, float* dgamma,
                                   float* dbeta, int G, int bpg, int C, const void* peers, int rank, int world,
                                   void* state, long long spin_limit, vfs_stream_t stream);
/* Round 6 - the exchange FOLDED into the apply passes of vfs_bn_act_fin_mask / vfs_bn_bwd_apply_fin (small row counts: the 16x16 /
 * 8x8 stages): `partial` holds the LOCAL statistics rows; the first workgroup of every 64-channel slab sums them, exchanges the
 * slab's G*2*64 sums with the peers' workgroups of the same slab through the windows and releases the slab's other workgroups, which
 * wait on a device-scope word instead of summing rows.  sums / bnp / running statistics (forward) and sums (backward) come from the
 * totals over the ranks, count = GLOBAL element count; dgamma / dbeta stay local sums.  Replaces vfs_bn_reduce_partials_xchg +
 * vfs_bn_act_fin (forward) and vfs_bn_bwd_sums_paramgrad_xchg + vfs_bn_bwd_apply (backward): one dependent launch less per BatchNorm
 * layer and direction - the SyncBN step costs what the single-GPU step costs plus the exchange latency.  G*2*min(C,64) <= 256
 * (two views), C <= 4096, G*2*C <= 8192.  state: (4 + 64) x uint64 in device memory, zero-initialised ({exchange counter, error
 * flag, workgroup ticket, chain counter, slab_ready[64]}); peers / rank / world / spin_limit as vfs_bn_reduce_partials_xchg.
 * seq (0 .. 4094) numbers the folded exchanges of one launch chain: the exchange's epoch is state[3] * 4096 + seq + 1, and every rank
 * must issue the same (chain, seq) sequence - vfs_p2p_chain_start(state) (one single-thread launch: state[3] += 1) goes to the head
 * of every chain that is recorded once and replayed (the recorded seq values repeat, the chain counter does not); a caller that
 * launches eagerly may simply count seq up and never start a chain.  Same torch call sites: SyncBatchNorm forward / backward
 * (configs/r*_*.py:9,15; apis/train.py:58-66). */
int vfs_p2p_chain_start(void* state, vfs_stream_t stream);
int vfs_bn_act_fin_xchg(const vfs_bf16* x, const float* partial, int bpg, const float* gamma, const float* beta, float* bnp,
                        double* sums, float* running_mean, float* running_var, const vfs_bf16* res, const vfs_bf16* rres,
                        const float* rbnp, vfs_bf16* y, uint8_t* mask_bits, long long M, int C, int mpg, int relu,
                        double count, float eps, float momentum, const void* peers, int rank, int world, void* state,
                        long long spin_limit, int seq, vfs_stream_t stream);
int vfs_bn_bwd_apply_fin_xchg(const vfs_bf16* g, const vfs_bf16* y, const vfs_bf16* x, const float* bnp, const float* partial,
                              int bpg, double* sums, float* dgamma, float* dbeta, vfs_bf16* dx, vfs_bf16* gm, long long M,
                              int C, int mpg, double count, int relu, const void* peers, int rank, int world, void* state,
                              long long spin_limit, int seq, vfs_stream_t stream);
int vfs_p2p_alloc(void** window);
int vfs_p2p_free(void* window);
int vfs_p2p_export(void* window, void* handle64);
int vfs_p2p_import(const void* handle64, void** window);
int vfs_p2p_unimport(void* window);
int vfs_p2p_allreduce_f64(double* buf, int n, const void* peers, int rank, int world, void* state, int phase,
                          long long spin_limit, vfs_stream_t stream);

/* ---- optimizer: torch.optim.SGD(lr, momentum, weight_decay) (configs/r*_*.py:134) on flat arenas --- */
/* skip_flag: NULL, or a device word (8 bytes) read when the kernel RUNS: non-zero -> the step changes nothing.  The trackers pass
 * the error word of the SyncBN window exchange (vfs_p2p_allreduce_f64's state[1]): a step whose statistics were poisoned by a
 * peer that never arrived must not reach the weights or the momentum (the host learns of it with the step's log values). */
int vfs_sgd_step(float* params, const float* grads, float* momentum_buf, long long n, float lr,
                 float momentum, float weight_decay, const void* skip_flag, vfs_stream_t stream);
int vfs_scale(float* x, long long n, float scale, vfs_stream_t stream);
/* ---- gradient clipping: optimizer_config = dict(grad_clip=dict(max_norm=..., norm_type=2)) (configs/r*_*.py:136), which
 * apis/train.py:85-93 hands to mmcv's OptimizerHook; OptimizerHook.clip_grads calls torch.nn.utils.clip_grad_norm_ on the trainable
 * parameters between loss.backward() and optimizer.step().  Here: one streaming reduction over the flat gradient arena, a finish
 * that leaves norm and coefficient in device memory, and an update that reads the coefficient there - no host read in the step.
 * norm_type: 2 or +infinity (anything else: VFS_ERR_ARG).
 *
 * vfs_grad_norm_rows: number of doubles in the partials buffer (host only; replaces nothing, it sizes the workspace).
 * vfs_grad_norm_partial (clip_grad_norm_'s per-tensor torch.norm calls, OptimizerHook.clip_grads): every one of the
 *   vfs_grad_norm_rows workgroups reduces its share of grads[0..n) (16-byte aligned; squares summed in double, or max |g|) and
 *   writes partials[workgroup] (accumulate == 0) or combines with the value there (accumulate != 0: the further contiguous ranges
 *   of trainable parameters).  One pass of the grid covers rows * 1024 floats.  No floating-point atomics: same bits on every run.
 * vfs_grad_norm_finish (clip_grad_norm_'s norm of norms and clip_coef_clamped): one workgroup combines the rows in a fixed
 *   order; out[0] = (float)total_norm, out[1] = (float)min(1, max_norm / (total_norm + 1e-6)); a NaN norm gives a NaN coefficient
 *   (torch with error_if_nonfinite=False).  max_norm > 0. */
int vfs_grad_norm_rows(int* rows);
int vfs_grad_norm_partial(const float* grads, long long n, float norm_type, double* partials, int accumulate, vfs_stream_t stream);
int vfs_grad_norm_finish(const double* partials, float norm_type, double max_norm, float* out, vfs_stream_t stream);
/* vfs_sgd_step with the gradient taken as grads[i] * (*clip) (clip_grad_norm_'s in-place g.mul_(clip_coef_clamped) of
 * OptimizerHook.clip_grads, folded into torch.optim.SGD.step; grads is NOT modified).  clip: device float, read when the kernel
 * runs (vfs_grad_norm_finish's out + 1).  *clip == 1.0 gives exactly vfs_sgd_step's bits.  skip_flag as above. */
int vfs_sgd_step_clip(float* params, const float* grads, float* momentum_buf, long long n, float lr, float momentum,
                      float weight_decay, const float* clip, const void* skip_flag, vfs_stream_t stream);
/* ---- optimizers with param groups: optimizer = dict(type='SGD' | 'Adam' | 'AdamW', ..., paramwise_cfg=...) (configs/r*_*.py:134-136),
 * which apis/train.py:72 hands to mmcv's build_optimizer: DefaultOptimizerConstructor makes one param group per parameter, torch's
 * optimizer then steps tensor by tensor.  Here one update launch covers every trainable range of the flat arena and every param group.
 *
 * vfs_opt_segment_map_words / vfs_opt_segment_map (host only, once per arena layout): `segments` is HOST memory, nseg x
 *   {begin, end, group} in words - the trainable parameters [begin, end) of the arena, sorted, inside [0, n), each beginning on a
 *   multiple of 4 words and none sharing a 16-byte vector with the one before (parameters are padded to 4 words), group in
 *   [0, ngroups).  The map (`words` ints, host memory) is what vfs_opt_step_table reads on the DEVICE: copy it there once.
 * vfs_opt_step_table (torch.optim.SGD.step / Adam.step / AdamW.step over all param groups): kind 0 SGD, 1 Adam, 2 AdamW, fp32.
 *   state1: momentum_buffer / exp_avg, state2: exp_avg_sq (NULL for SGD); params, grads and the states are arenas of n words with
 *   the same layout, 16-byte aligned.  map: the DEVICE copy of vfs_opt_segment_map's output for this (n, nseg).  hyper: HOST
 *   memory, ngroups x 8 floats, read before the call returns: {lr, weight_decay, momentum} for SGD, {lr, weight_decay, beta1, beta2,
 *   eps} for Adam / AdamW (the other slots are ignored; the bias corrections of `step` are worked out inside).  Up to 224
 *   groups the rows are kernel arguments of the update launch itself; more go through `table` (device workspace of ngroups x 8
 *   floats, 16-byte aligned, always required), written on `stream` by two small launches in front of the update with the
 *   values of THIS call.  Nothing waits for a copy, a changed lr holds from this step on.  At most 448 param groups.
 *   SGD: g' = clip g + wd p; buf = momentum buf + g'; p -= lr (nesterov ? g' + momentum buf : buf)   (dampening 0; a zero buffer
 *   gives torch's first step).  Adam (amsgrad off): the wd p term joins the gradient.  AdamW: p *= 1 - lr wd before the moments.
 *   step: torch's state['step'] AFTER this update (>= 1; ignored by SGD).  clip: NULL or the device coefficient of
 *   vfs_grad_norm_finish, skip_flag: NULL or the device word, both as in vfs_sgd_step_clip.  Words outside every segment are
 *   neither read nor written.  One group without nesterov gives vfs_sgd_step's / vfs_sgd_step_clip's bits. */
int vfs_opt_segment_map_words(long long n, int nseg, long long* words);
int vfs_opt_segment_map(const long long* segments, int nseg, long long n, int ngroups, int* map, long long words);
int vfs_opt_step_table(int kind, float* params, const float* grads, float* state1, float* state2, long long n, const int* map, int nseg,
                       const float* hyper, int ngroups, float* table, int nesterov, int step, const float* clip, const void* skip_flag,
                       vfs_stream_t stream);
/* x[0..n) *= *coef, coef a device float read when the kernel runs (clip_grad_norm_'s g.mul_(clip_coef_clamped) for a caller that
 * drives the loop itself, OptimizerHook.clip_grads); x 16-byte aligned */
int vfs_scale_by(float* x, long long n, const float* coef, vfs_stream_t stream);
/* bf16 gradient buckets for the data-parallel all-reduce (opt-in, VFS_GRAD_BF16=1; the reference's DDP - apis/train.py:62-66 -
 * reduces fp32): dst = bf16(src * scale) before the collective, dst = float(src) after it; buffers 16-byte aligned */
int vfs_f32_to_bf16(const float* src, vfs_bf16* dst, long long n, float scale, vfs_stream_t stream);
int vfs_bf16_to_f32(const vfs_bf16* src, float* dst, long long n, vfs_stream_t stream);

/* ---- DAVIS label propagation (VanillaTracker.forward_test, vanilla_tracker.py:80-206) -------
 * F.normalize(dim=channel) of NHWC rows, once per frame when it enters the bank
 * (local_attention.py:277-279 does it on every propagation step) */
int vfs_l2norm_rows(const vfs_bf16* x, vfs_bf16* y, long long P, int C, vfs_stream_t stream);
/* masked_attention_efficient (local_attention.py:237-348) + spatial_neighbor 'circle'
 * (affinity_utils.py:144-156): fbank [frames][H*W][C] normalised bf16, sbank [frames][H*W][CO]
 * fp32; key frames kslot[0..nkeys) in the reference's order (first frame first, duplicates
 * allowed); out [H*W][CO].  radius = neighbor_range // 2 (<= 0: no mask), the first non_mask_len
 * key frames are never masked (test_cfg.with_first_neighbor=False -> 1), topk <= 10, nkeys <= 64,
 * C % 64 == 0.  workspace: at least vfs_labelprop_workspace_bytes(H, W) bytes (per-split partial top-k lists - key frames,
 * and for vfs_labelprop_f32 the 64-key blocks of a frame's window as well, are split over workgroups because a DAVIS
 * frame has only 8x14 query tiles); workspace_bytes = what the caller allocated: a smaller buffer is REFUSED
 * (VFS_ERR_ARG) instead of written past (the size grew between library versions - ABI version 2) */
int vfs_labelprop_workspace_bytes(int H, int W, long long* bytes);
int vfs_labelprop(const vfs_bf16* fbank, const float* sbank, float* out, void* workspace, long long workspace_bytes, int qframe,
                  const int* kslot, int nkeys, int H, int W, int C, int CO, int radius, int non_mask_len,
                  int topk, float temperature, vfs_stream_t stream);
/* bilinear upsample (align_corners=False) + per-channel min-max normalisation where max > 0 +
 * argmax -> uint8 [Ho][Wo] (vanilla_tracker.py:162-181); partial: workspace float[64*CO*2] */
int vfs_seg_postprocess(const float* seg, float* partial, uint8_t* label, int H, int W, int CO, int Ho,
                        int Wo, vfs_stream_t stream);
/* F.one_hot of the resized first-frame label map into the seg bank (vanilla_tracker.py:96-100) */
int vfs_onehot(const uint8_t* labels, float* out, int P, int CO, vfs_stream_t stream);

/* split-K partials of MANY layers -> their gradients in ONE launch.  desc: device array of nrecords 56-byte records
 * {const float* partial; float* grad; int nsplit, Cout, Ktot, Cin, KH, KW, stem, block_start, nblocks, pad;} (stem = 1:
 * the 7x7 stem's k-layout, Ktot 256 for vfs_stem_wgrad / 224 for vfs_stem_wgrad_fused with Cin = 3); a record is served
 * by workgroups [block_start, block_start + nblocks), 128 elements each per pass; total_blocks = sum of nblocks.
 * grad += sum over the splits in a fixed order (deterministic). */
int vfs_wgrad_reduce_table(const void* desc, int nrecords, int total_blocks, vfs_stream_t stream);

/* ---- fp32 evaluation path ("exact" precision; csrc/exact_f32.hip) ------------------------------------
 * The reference evaluates in fp32 and its outputs are INTEGER label maps, so the default forward_test path stores
 * and computes in fp32 with bit-defined arithmetic: every dot product is one ascending chain acc = fma(a_k, b_k, acc)
 * on v_mfma_f32_32x32x2_f32, every other step a single correctly rounded fp32 operation, exp() an explicit
 * polynomial, top-k ties to the lowest candidate index.  oracle/exact_oracle.c states the same arithmetic in C and
 * the results agree bit for bit (tests/test_exact_f32.py); the bf16 entry points above remain as the fast mode.
 *
 * mmcv ConvModule in eval mode (conv -> BN(running statistics) [-> + identity] [-> ReLU]; resnet.py:51-73,102-111,
 * 163-191,221-230): y[N,Ho,Wo,Cout] = [relu]( fma(conv(x, w), scale, shift) [+ res] ), fp32 NHWC, w [Cout][KH][KW][Cin]
 * (the chain runs kh, kw, cin ascending), Cin % 4 == 0 (3-channel frames as NHWC4 with zero weights on channel 3),
 * scale/shift [Cout] or both NULL, any stride / padding / dilation */
int vfs_conv_f32_fwd(const float* x, const float* w, const float* scale, const float* shift, const float* res, float* y,
                     int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                     int dilation, int relu, vfs_stream_t stream);
/* imgs fp32 [B][V][3][T][H][W] -> fp32 NHWC4 frames out[(v*B+b)*T+t][h][w][4], channel 3 = 0 (common/utils.py:45-53) */
int vfs_imgs_to_nhwc4_f32(const float* imgs, float* out, int B, int V, int T, int H, int W, vfs_stream_t stream);
/* nn.MaxPool2d(3, 2, 1) (resnet.py:435), fp32 NHWC, C % 4 == 0 */
int vfs_maxpool_f32(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo, vfs_stream_t stream);
/* F.normalize(dim=channel, eps=1e-12) of fp32 rows [P][C] (local_attention.py:277-279), C % 4 == 0 */
int vfs_l2norm_rows_f32(const float* x, float* y, long long P, int C, vfs_stream_t stream);
/* vfs_labelprop on an fp32 bank: score = chain(key . query) / temperature, top-k by (score desc, candidate id asc) with
 * id = key_position * H*W + pixel, softmax weights exp(s - s_max) / sum in sorted order; the first non_mask_len key
 * frames are not masked (test_cfg.with_first_neighbor=False -> 1, local_attention.py:303-309); workspace as vfs_labelprop */
int vfs_labelprop_f32(const float* fbank, const float* sbank, float* out, void* workspace, long long workspace_bytes, int qframe,
                      const int* kslot, int nkeys, int H, int W, int C, int CO, int radius, int non_mask_len, int topk,
                      float temperature, vfs_stream_t stream);
/* Two-pass form of vfs_labelprop_f32 with IDENTICAL results (csrc/labelprop2.hip): every in-window candidate is first scored on the
 * bf16 matrix path from a split copy of the bank (x = hi + lo, three products; |s~ - s| <= 3 * 2^-16 + 4 * C * 2^-24 for unit
 * rows), the candidates within twice that bound of the query's 10th-best s~ - the only ones that can be in the exact top 10 -
 * are rescored with the defining fp32 chain and go through the same total order / softmax / value sum.
 *   vfs_split_rows_bf16x2: hl [P][C/16][16 hi | 16 lo] bf16 from unit rows x [P][C] fp32 (C % 16 == 0), once per frame;
 *   vfs_labelprop_f32_2pass: hlbank = the split copy of fbank (same frame indexing).  unit_rows = 0 (test_cfg.with_norm=False),
 *   hlbank = NULL or C not in {256, 512, 1024} -> the dense kernel; a candidate list that overflows -> the dense kernel redoes
 *   the frame, decided on the device.  workspace: vfs_labelprop_f32_2pass_workspace_bytes(H, W) for the full list capacity (4608
 *   entries per query: 237 MB at 60 x 107), or vfs_labelprop_f32_2pass_workspace_bytes_for(H, W, entries_per_query >= 16) - the launch
 *   derives the capacity from workspace_bytes; fewer entries trade memory for dense redos of the first frames of a clip. */
int vfs_split_rows_bf16x2(const float* x, vfs_bf16* hl, long long P, int C, vfs_stream_t stream);
int vfs_labelprop_f32_2pass_workspace_bytes(int H, int W, long long* bytes);
int vfs_labelprop_f32_2pass_workspace_bytes_for(int H, int W, int entries_per_query, long long* bytes);
int vfs_labelprop_f32_2pass(const float* fbank, const vfs_bf16* hlbank, const float* sbank, float* out, void* workspace,
                            long long workspace_bytes, int qframe, const int* kslot, int nkeys, int H, int W, int C, int CO,
                            int radius, int non_mask_len, int topk, float temperature, int unit_rows, vfs_stream_t stream);
/* F.interpolate(mode='bilinear', align_corners=False) of a C-channel fp32 map between layouts (NCHW [C][H][W] or NHWC
 * [H][W][C], chosen per side): one-hot reference maps -> feature resolution, soft label maps -> original resolution
 * (vanilla_tracker.py:101-111,162-166 when ref_seg_map is 4-D) */
int vfs_bilinear_resize_f32(const float* src, float* dst, int C, int H, int W, int Ho, int Wo, int src_nhwc, int dst_nhwc,
                            vfs_stream_t stream);
/* vfs_seg_postprocess with every step a single fp32 operation (no contraction) */
int vfs_seg_postprocess_exact(const float* seg, float* partial, uint8_t* label, int H, int W, int CO, int Ho, int Wo,
                              vfs_stream_t stream);
/* ---- label propagation of a BATCH of videos in lock-step (VanillaTracker.forward_test_batch) ----
 * Up to 64 slots of one frame size advance together: one call of vfs_labelprop_f32_batch / vfs_labelprop_f32_2pass_batch is one
 * propagation step of EVERY slot in the launches one video takes (the grids carry a slot dimension), each slot at its own query
 * frame with its own key list and class count, and every slot's output has the bits of the single-video call.
 *   banks     fbank [nslots][Tcap][H*W][C] fp32, hlbank [nslots][Tcap][H*W][2C] (vfs_split_rows_bf16x2 of fbank),
 *             sbank [nslots][Tcap][H*W][COcap] fp32: slot n starts at n * Tcap * H*W * COcap and holds its label rows PACKED with
 *             its own class count, [frame][H*W][CO_n].  The output of a step is frame `qframe` of the slot's label rows.
 *   desc      device pointer to the rows of THIS step, int32 [nslots][VFS_LPB_DESC_INTS]: [0] active (0: the slot's workgroups
 *             leave at once, nothing of the slot is read or written), [1] qframe, [2] nkeys, [3] non_mask_len, [4] CO_n,
 *             [5] map position (read by the post-processing only, below; the propagation kernels do not read it), [6..7] reserved
 *             (0), [8..71] key frames (frame indices inside the slot, reference order).  A caller that knows every clip's length
 *             writes the rows of all steps once ([steps][nslots][VFS_LPB_DESC_INTS]) and passes row block `step`: nothing is copied
 *             to the device inside the step loop.  A row outside the single-video ranges (qframe / key frames < Tcap, 1 <= nkeys <=
 *             max_nkeys, 0 <= non_mask_len < nkeys, 1 <= CO_n <= COcap) is treated as inactive.
 *   host side nactive = active rows of this step (the key-frame splits are chosen for that many videos sharing the chip),
 *             max_nkeys >= every active row's nkeys (sizes the grids).
 *   workspace per slot, as the single-video calls: vfs_labelprop_f32_batch_workspace_bytes(H, W, nslots);
 *             vfs_labelprop_f32_2pass_batch_workspace_bytes(H, W, entries_per_query, nslots) (0 = the full list capacity) =
 *             256 bytes of per-slot overflow words (int32 [nslots]: 1 = the slot's lists overflowed and the dense kernels redid THAT
 *             slot, decided on the device; the other slots are not touched) + nslots regions in the single-video layout.
 *   vfs_labelprop_f32_2pass_batch runs the dense kernels for every slot when hlbank = NULL, unit_rows = 0 or C is not 256 / 512 / 1024.
 * vfs_seg_postprocess_exact_batch / vfs_bilinear_resize_f32_batch: the per-step post-processing of every active slot in one launch
 * set, from frame qframe ([1]) of the slot's label rows into the map position ([5]) of the slot's maps.  The maps have Tmaps
 * positions per slot, whatever Tcap is (a ring bank of a few positions feeds the maps of a whole clip): preds uint8
 * [nslots][Tmaps][Ho*Wo] label maps (partial: fp32 [nslots][64][COcap][2]), or fp32 soft maps, slot n at n * Tmaps * COcap * Ho*Wo
 * holding [map position][CO_n][Ho][Wo] packed.  A row whose map position is outside [0, Tmaps), whose qframe is outside [0, Tcap)
 * or whose CO_n is outside [1, COcap] is inactive for the post-processing: nothing of the slot is written. */
#define VFS_LPB_DESC_INTS 72
int vfs_labelprop_f32_batch_workspace_bytes(int H, int W, int nslots, long long* bytes);
int vfs_labelprop_f32_batch(const float* fbank, float* sbank, void* workspace, long long workspace_bytes, const int* desc, int nslots,
                            int nactive, int max_nkeys, int Tcap, int H, int W, int C, int COcap, int radius, int topk,
                            float temperature, vfs_stream_t stream);
int vfs_labelprop_f32_2pass_batch_workspace_bytes(int H, int W, int entries_per_query, int nslots, long long* bytes);
int vfs_labelprop_f32_2pass_batch(const float* fbank, const vfs_bf16* hlbank, float* sbank, void* workspace, long long workspace_bytes,
                                  const int* desc, int nslots, int nactive, int max_nkeys, int Tcap, int H, int W, int C, int COcap,
                                  int radius, int topk, float temperature, int unit_rows, vfs_stream_t stream);
int vfs_seg_postprocess_exact_batch(const float* sbank, float* partial, uint8_t* preds, const int* desc, int nslots, int Tcap, int Tmaps,
                                    int H, int W, int COcap, int Ho, int Wo, vfs_stream_t stream);
int vfs_bilinear_resize_f32_batch(const float* sbank, float* preds, const int* desc, int nslots, int Tcap, int Tmaps, int H, int W,
                                  int COcap, int Ho, int Wo, vfs_stream_t stream);
/* The same lock-step for the bf16 kernels (test_cfg.precision = 'bf16'): vfs_labelprop_batch is one step of vfs_labelprop in every
 * slot, vfs_seg_postprocess_batch one vfs_seg_postprocess of every active slot's propagated frame (soft maps: vfs_bilinear_resize_f32_batch,
 * which does not depend on the precision).  Banks, descriptor rows, preds and partial as above, with fbank bf16 [nslots][Tcap][H*W][C]
 * and no split copy; workspace per slot: vfs_labelprop_batch_workspace_bytes(H, W, nslots).  The bf16 top-k keeps the first of equal
 * scores, so the order candidates arrive in belongs to the result: every slot splits its key frames over workgroups exactly as
 * vfs_labelprop does for that slot's nkeys, whatever nactive and max_nkeys are (max_nkeys sizes the grid), and its output has the bits
 * of the single-video call.  Limits as vfs_labelprop: C % 64 == 0, topk <= 10, max_nkeys <= 64. */
int vfs_labelprop_batch_workspace_bytes(int H, int W, int nslots, long long* bytes);
int vfs_labelprop_batch(const vfs_bf16* fbank, float* sbank, void* workspace, long long workspace_bytes, const int* desc, int nslots,
                        int nactive, int max_nkeys, int Tcap, int H, int W, int C, int COcap, int radius, int topk, float temperature,
                        vfs_stream_t stream);
int vfs_seg_postprocess_batch(const float* sbank, float* partial, uint8_t* preds, const int* desc, int nslots, int Tcap, int Tmaps, int H,
                              int W, int COcap, int Ho, int Wo, vfs_stream_t stream);
/* ---- table-driven ingest of a feature bank: ring banks and streaming (csrc/bank_ingest.hip) ----
 * For query frame f the reference reads frame 0 and frames max(0, f - precede_frames) .. f - 1 only (vanilla_tracker.py:132-149):
 * a bank of precede_frames + 2 positions per video serves a clip of any length, and a frame can enter it when it arrives.  One
 * call stores the feature maps of n images (one new frame of every video of a step) in ONE launch, each image at its own place:
 *   feats     [n][P][C], the maps as the backbone leaves them (P = H*W rows of C channels per image), fp32 / bf16;
 *   fbank     [bank_rows][C] in the type of feats, hlbank [bank_rows][2C] or NULL (fp32 only);
 *   table     device pointer, long long [n][2]: image i goes to rows table[2i] .. table[2i] + P of fbank and to rows table[2i + 1] ..
 *             of hlbank (ignored without hlbank).  An image whose rows do not lie inside [0, bank_rows) is left out, nothing of it
 *             is written.  Destinations must not overlap.
 *   unit_rows 1: a row of fbank = vfs_l2norm_rows_f32 (vfs_l2norm_rows) of the feature row and a row of hlbank =
 *             vfs_split_rows_bf16x2 of that, bit for bit: the same code; every feature row is read once.  0 (test_cfg.with_norm=False):
 *             a plain copy, and hlbank must be NULL.
 * VFS_ERR_SHAPE: n outside 1 .. 65535, P < 1, bank_rows < P, C % 4 (bf16: C % 8), C > 2048 (a row is held in registers), C % 16
 * with hlbank, feature maps or banks not 16-byte aligned. */
int vfs_bank_ingest_f32(const float* feats, float* fbank, vfs_bf16* hlbank, const long long* table, int n, long long P, int C,
                        long long bank_rows, int unit_rows, vfs_stream_t stream);
int vfs_bank_ingest_bf16(const vfs_bf16* feats, vfs_bf16* fbank, const long long* table, int n, long long P, int C, long long bank_rows,
                         int unit_rows, vfs_stream_t stream);

/* ---- DAVIS-2017 semi-supervised J&F (datasets/davis_dataset.py:68-140 -> davis2017.evaluation) -----
 * pred / gt: uint8 label maps [T][H][W]; frames 1..T-2 are evaluated (first = given, last excluded);
 * objects 1..nobj (<= 32), gt label 255 = void when use_void; radius = ceil(0.008*||(H,W)||) of the
 * boundary-match disk.  counts: int32 [T-2][nobj][6] = {|pred&gt|, |pred|gt|, #pred boundary,
 * #gt boundary, matched pred boundary, matched gt boundary}; scratch: uint32 [2][T-2][H][W].
 * J = c0/c1 (1 if c1 == 0); F from c2..c5 with the package's empty-boundary conventions. */
int vfs_davis_counts(const uint8_t* pred, const uint8_t* gt, int* counts, void* scratch, int T, int H, int W,
                     int nobj, int radius, int use_void, vfs_stream_t stream);

/* ---- JHMDB pose (PCK) and VIP parts (mIoU): the other two label-propagation benchmarks -------------
 * vfs_heatmap_topk: JHMDBDataset.img2coord (datasets/jhmdb_dataset.py:118-136) without the np.argsort over every
 * full-resolution map.  maps fp32 [N][H*W] (N = frames x key points of the tracker's [T][K][H][W]; 4-byte aligned,
 * any H*W <= 2^28), topk 1..8 (the reference: 5), H*W >= topk (else VFS_ERR_SHAPE).  Per map: vals fp32 [N][topk]
 * and idx int32 [N][topk] = the topk largest values and their flat indices in ASCENDING rank order (what
 * argsort(...)[-topk:] yields); larger value ranks higher, among equal values the LOWER flat index ranks higher
 * (argsort leaves ties open); minv fp32 [N] = the map's minimum; flags int32 [N]: bit 0 = every element is zero,
 * bit 1 = the map holds a NaN, bit 2 = the map holds a -inf (elements equal to -inf never rank, so a map with fewer than
 * topk elements above -inf has no defined top-k).  Both are bad data, not a bad call: VFS_OK, and vals / idx of that map
 * mean nothing (minv is the minimum over the non-NaN elements). */
int vfs_heatmap_topk(const float* maps, float* vals, int* idx, float* minv, int* flags, long long N, int H, int W, int topk,
                     vfs_stream_t stream);
/* vfs_label_counts: intersect_and_union (core/evaluation/iou.py:5-63) of one frame or of a whole video.  pred / gt uint8 [n]
 * (n <= 2^40), num_classes 1..256, ignore_index 0..255 or -1 for none.  counts uint64 [num_classes][3] = {intersect,
 * prediction area, label area} (union = prediction + label - intersect), ADDED onto what the buffer holds: zero it once,
 * sum a dataset on the device, read it back once.  Pixels with gt == ignore_index are dropped first.  As
 * np.histogram(x, bins=np.arange(num_classes + 1)), whose last bin is closed: a value equal to num_classes is counted in
 * class num_classes - 1, larger values are dropped. */
int vfs_label_counts(const uint8_t* pred, const uint8_t* gt, unsigned long long* counts, long long n, int num_classes,
                     int ignore_index, vfs_stream_t stream);
/* vfs_pose_heatmaps: the pose_coord branch of RawFrameDecode + draw_label_map (pipelines/loading.py:1055-1101).  patch fp32
 * [P][P] (P = 6*sigma + 1 <= 1024): exp(-((x-x0)^2 + (y-y0)^2) / (2 sigma^2)) evaluated in float64 on the host and rounded
 * to fp32 (sigma <= 0: P = 1, patch = {1}); kp int32 [K][5] per key point = {ul_x, ul_y, br_x, br_y, inside}: the reference's
 * int()-truncated corners and the outcome of its early-return test.  out fp32 [K][H][W] (H*W <= 2^30, K <= 65535) is
 * written whole: zero, and out[k][y][x] = patch[y - ul_y][x - ul_x] for max(0, ul) <= (x, y) < min(br, (W, H)) when inside. */
int vfs_pose_heatmaps(const float* patch, const int* kp, float* out, int K, int H, int W, int P, vfs_stream_t stream);

/* ---- training input pipeline (configs/r*_*.py:48-91: RandomResizedCrop -> Resize -> Flip -> Normalize ->
 * FormatShape NCTHW; pipelines/augmentations.py:171-334,487-596,600-707,711-794) in one pass over the decoded
 * frames.  src uint8 [B*V*T][Hs][Ws][3] RGB in pipeline order (b, v, t); boxes int32 [F][4] = left, top,
 * right, bottom; flips uint8 [F]; outputs (either may be NULL): imgs fp32 [B][V][3][T][Ho][Wo] (what
 * train_step takes), x4 bf16 NHWC4 [V*B*T][Ho][Wp][4] (what vfs_stem_fwd reads).  Bilinear = cv2.resize
 * INTER_LINEAR on 8-bit data (fixed point), normalisation = mmcv.imnormalize_ (double arithmetic). */
int vfs_crop_resize_flip_norm(const uint8_t* src, const int* boxes, const uint8_t* flips, float* imgs, vfs_bf16* x4,
                              int B, int V, int T, int Hs, int Ws, int Ho, int Wo, int Wp, double mean_r,
                              double mean_g, double mean_b, double std_r, double std_g, double std_b,
                              vfs_stream_t stream);

/* the same chain with the photometric steps of the object-level configs between Flip and Normalize
 * (r18_sgd_cos_100e_r2_1xNx8_k400.py / r50_sgd_cos_100e_r5_1xNx2_k400.py train_pipeline; pipelines/augmentations.py:1224-1320
 * ColorJitter, RandomGrayScale, RandomGaussianBlur), applied to the uint8 frame after the resize and flip, in that order.
 * photo int32 [F][8], one row per frame (pipeline order (b, v, t)):
 *   [0] jitter ops in application order, op k in bits 4k..4k+3 (k = 0..3): 1 brightness, 2 contrast, 3 saturation,
 *       4 hue, 0 none.  0 = ColorJitter not applied to the frame (its shuffled order, torchvision 0.7 get_params)
 *   [1] [2] [3] brightness / contrast / saturation factors as fp32 bits: PIL ImageEnhance = Image.blend(degenerate,
 *       img, factor) with degenerate 0 / the frame's mean PIL luma int(mean + 0.5) when contrast runs / the pixel's luma
 *   [4] bits 0..7: hue shift added to PIL's uint8 H, mod 256 (= np.uint8(hue_factor * 255) of torchvision 0.7 adjust_hue);
 *       bits 8..15: r, the integer part of the blur's box radius.  Read by the _blur entry points only, which clamp it to
 *       their max_blur_radius; vfs_crop_resize_flip_photo_norm and its _ragged form ignore bits 8 and up (r = 0)
 *   [5] grey flag: mmcv.rgb2gray = cv2 RGB2GRAY fixed point (R*4899 + G*9617 + B*1868 + 8192) >> 14, to 3 channels
 *   [6] [7] blur ww, fw: PIL GaussianBlur(radius=sigma) = an extended box blur of fp32 radius rad, r = int(rad):
 *       ww = int(2^24 / (2*rad + 1)) in fp32, fw = (2^24 - (2*r + 1) * ww) / 2; one pass along a line of n pixels is
 *       out[x] = (ww * sum_{|d| <= r} in[clamp(x+d)] + fw * (in[clamp(x-r-1)] + in[clamp(x+r+1)]) + 2^23) >> 24 with
 *       clamp(i) = min(max(i, 0), n-1), per channel, uint8 after every pass; three horizontal then three vertical passes.
 *       ww = 0: no blur.  Larger values are clamped: ww to 2^24 / (2*r + 1), fw to (2^24 - (2*r + 1) * ww) / 2
 *   A row with r = 0 (every row written before the radius existed) means the same to all four entry points.
 * Frames whose row is all zero come out bit-identical to vfs_crop_resize_flip_norm.  workspace: at least
 * vfs_crop_resize_flip_photo_norm_workspace_bytes(B*V*T, Ho, Wo) bytes ([F] luma sums, [F][Ho][Wo] uint8 RGBX frames),
 * workspace_bytes = what the caller allocated: a smaller buffer is REFUSED.  Other arguments as vfs_crop_resize_flip_norm. */
int vfs_crop_resize_flip_photo_norm_workspace_bytes(int frames, int Ho, int Wo, long long* bytes);
int vfs_crop_resize_flip_photo_norm(const uint8_t* src, const int* boxes, const uint8_t* flips, const int* photo,
                                    void* workspace, long long workspace_bytes, float* imgs, vfs_bf16* x4, int B, int V,
                                    int T, int Hs, int Ws, int Ho, int Wo, int Wp, double mean_r, double mean_g,
                                    double mean_b, double std_r, double std_g, double std_b, vfs_stream_t stream);
/* the photometric chain for blurs of box radius 1 and above (sigma_range (0.1, 2.0) of the SimSiam / BYOL recipes reaches
 * 1.375).  max_blur_radius (0..3, else VFS_ERR_SHAPE) = the largest r a row of this launch may carry; it selects the
 * second launch's tile (halo 3 * (max_blur_radius + 1) pixels), so a caller that keeps it fixed runs the same launches
 * whatever radii a batch drew.  0 launches exactly what vfs_crop_resize_flip_photo_norm launches.  Same workspace. */
int vfs_crop_resize_flip_photo_norm_blur(const uint8_t* src, const int* boxes, const uint8_t* flips, const int* photo,
                                         void* workspace, long long workspace_bytes, float* imgs, vfs_bf16* x4, int B,
                                         int V, int T, int Hs, int Ws, int Ho, int Wo, int Wp, double mean_r,
                                         double mean_g, double mean_b, double std_r, double std_g, double std_b,
                                         int max_blur_radius, vfs_stream_t stream);

/* the same two chains for a batch whose samples were decoded at different sizes: the reference crops and resizes sample by
 * sample, each at its own img_shape (pipelines/augmentations.py:171-334,487-596), and DecordDecode hands it every Kinetics
 * video at its own size (340x256, 454x256, 256x340, ...).  src is a byte buffer of src_bytes bytes; srcdesc int32 [B][4],
 * one row per SAMPLE = {offset low 32 bits, offset high 32 bits, Hs, Ws}: the V*T frames of sample b lie contiguously as
 * uint8 [V*T][Hs_b][Ws_b][3] at src + offset_b in pipeline order (v, t); byte offsets, no alignment required.  boxes are
 * clamped to the sample's own Hs_b, Ws_b.  Guard: a row with Hs <= 0, Ws <= 0, a negative offset or
 * offset + V*T*Hs*Ws*3 > src_bytes makes its sample invalid: nothing is read for it and every output element it owns (imgs,
 * x4, the x4 pad column) is zero; the other samples of the launch are unaffected.  So no table can make the kernels read
 * outside [src, src + src_bytes).  src_bytes <= 0 is refused like a null src.  Everything else - the arithmetic, boxes,
 * flips, photo, the workspace rule, the outputs, the frame cap - as the uniform entry points; a batch of equal sizes laid
 * out back to back gives their bits. */
int vfs_crop_resize_flip_norm_ragged(const uint8_t* src, long long src_bytes, const int* srcdesc, const int* boxes,
                                     const uint8_t* flips, float* imgs, vfs_bf16* x4, int B, int V, int T, int Ho, int Wo,
                                     int Wp, double mean_r, double mean_g, double mean_b, double std_r, double std_g,
                                     double std_b, vfs_stream_t stream);
int vfs_crop_resize_flip_photo_norm_ragged(const uint8_t* src, long long src_bytes, const int* srcdesc, const int* boxes,
                                           const uint8_t* flips, const int* photo, void* workspace,
                                           long long workspace_bytes, float* imgs, vfs_bf16* x4, int B, int V, int T,
                                           int Ho, int Wo, int Wp, double mean_r, double mean_g, double mean_b,
                                           double std_r, double std_g, double std_b, vfs_stream_t stream);
/* vfs_crop_resize_flip_photo_norm_blur for a batch of mixed frame sizes */
int vfs_crop_resize_flip_photo_norm_blur_ragged(const uint8_t* src, long long src_bytes, const int* srcdesc,
                                                const int* boxes, const uint8_t* flips, const int* photo, void* workspace,
                                                long long workspace_bytes, float* imgs, vfs_bf16* x4, int B, int V, int T,
                                                int Ho, int Wo, int Wp, double mean_r, double mean_g, double mean_b,
                                                double std_r, double std_g, double std_b, int max_blur_radius,
                                                vfs_stream_t stream);

/* ---- SiamFC probe head (projects/siamfc-pytorch/siamfc/heads.py:16-23,51-58 `_fast_xcorr`): response maps
 * out[m][i][j] = scale * sum_{u,v,c} z[m % nz][u][v][c] * x[m][i+u][j+v][c]; z bf16 [nz][Hz][Wz][C], x bf16 [nx][H][W][C] (NHWC),
 * out fp32 [nx][H-Hz+1][W-Wz+1]; nx % nz == 0, C % 8 == 0.  Forward only (inference of a trained probe). */
int vfs_xcorr_fwd(const vfs_bf16* z, const vfs_bf16* x, float* out, int nz, int nx, int Hz, int Wz, int H, int W, int C,
                  float scale, vfs_stream_t stream);

/* training the probe (siamfc_tracker_base.py:364-387 `train_step`): backward of the cross-correlation.  g fp32
 * [nx][H-Hz+1][W-Wz+1] = dL/d(responses); dz bf16 [nz][Hz][Wz][C] (summed over the search features that share an exemplar),
 * dx bf16 [nx][H][W][C]; either may be NULL.  The gradients feed vfs_conv_wgrad / vfs_bias_grad of the 1x1 convs. */
int vfs_xcorr_bwd(const vfs_bf16* z, const vfs_bf16* x, const float* g, vfs_bf16* dz, vfs_bf16* dx, int nz, int nx, int Hz, int Wz,
                  int H, int W, int C, float scale, vfs_stream_t stream);
/* the probe's losses on n response values (projects/siamfc-pytorch/siamfc/losses.py): mode 0 BalancedLoss (:24-41, param =
 * neg_weight), mode 1 FocalLoss (:44-65, param = gamma; the normaliser mean(avg_weight) is differentiated through, as autograd
 * does).  loss[0] = value; grad (may be NULL) = scale * dL/d(responses). */
int vfs_siamfc_loss(const float* responses, const float* labels, float* loss, float* grad, int n, int mode, float param, float scale,
                    vfs_stream_t stream);
/* torch.optim.Adam (amsgrad off; default_config_base.py:33, siamfc_tracker_base.py:139-145) on flat fp32 arrays, step >= 1 */
int vfs_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, vfs_stream_t stream);

/* ---- SiamFC probe, tracking loop (siamfc_tracker_base.py:222-297 `update`): the per-frame work around the backbone and the
 * cross-correlation.  The three entry points restate, operation by operation, what vfs_amd/siamfc.py computes on the host
 * (crop_and_resize, resize_cubic, the tail of SiamFCProbe.update); every reduction has a fixed order.
 *
 * vfs_siamfc_crops: S <= 8 square crops of one frame.  frame uint8 [H][W][3] (RGB, device); out fp32 [S][3][out_size][out_size],
 * values 0..255 (what the probe feeds to its backbone).  params: int32 [S][12] in HOST memory (read before the call returns,
 * passed on as kernel arguments), one row per crop, computed by the host in float64 as crop_and_resize does:
 *   [0] valid (0: the crop is all zeros - empty in-image patch or negative pad)   [1] [2] x, y origin of the in-image patch
 *   [3] [4] its width, height   [5] [6] its width, height after the resize   [7] [8] x, y where it lands in the crop
 *   [9] [10] [11] fill colour clip(rint(average colour)) of the rest
 * The patch is resized by OpenCV's 8-bit bilinear arithmetic (11-bit coefficients rint(fr * 2048), >> 4, >> 16, (x + 2) >> 2,
 * clamped to 0..255), evaluated per output pixel.  A row whose patch or target rectangle leaves its array is REFUSED. */
int vfs_siamfc_crops(const uint8_t* frame, const int* params, float* out, int H, int W, int S, int out_size, vfs_stream_t stream);
/* vfs_siamfc_upsample: responses fp32 [S][r][r] -> up_out fp32 [S][up][up], Keys cubic (A = -0.75) with the caller's taps:
 * tap_idx int32 [up][4] (indices into a row / column, border replicated), tap_w fp32 [up][4], both 16-byte aligned and used for
 * both axes; horizontal pass then vertical pass, each value ((p0 + p1) + p2) + p3 of four rounded fp32 products (no fused
 * multiply-add).  Every value is multiplied by penalty[s] (fp32 [S]).  scale_max [S]: the maximum of each penalised map as a
 * 64-bit key - high half the float mapped to an order-preserving unsigned integer, low half 0xffffffff - flat index (the
 * lowest index of the maximum wins); consumed by vfs_siamfc_peak.  r * r <= 1024. */
int vfs_siamfc_upsample(const float* responses, const int* tap_idx, const float* tap_w, const float* penalty, float* up_out,
                        unsigned long long* scale_max, int S, int r, int up, vfs_stream_t stream);
/* vfs_siamfc_peak (one workgroup): scale_id = the scale with the largest maximum (lowest on ties); on that map x:
 * x - min(x) in fp32, its sum in fp64 rounded to fp32, (x - min) / (sum + 1e-16) in fp32, times one_minus_wi in fp32, plus
 * window_influence * hann[i] in fp64 (hann fp64 [up][up], the normalised Hann window); argmax with the lowest flat index on
 * ties.  record int32 [4] (16-byte aligned) = {scale_id, row, col, 0}. */
int vfs_siamfc_peak(const float* up_in, const unsigned long long* scale_max, const double* hann, int* record, int S, int up,
                    float one_minus_wi, double window_influence, vfs_stream_t stream);


/* ---- SiamFC probe, tracking loop for a batch of sequences: the tracker state on the device, N <= 64 slots in lock-step (a slot
 * holds one sequence at a time).  Per slot n:
 *   state    fp64  [N][8] = {center_y, center_x, target_h, target_w, z_sz, x_sz, 0, 0}.  center and target_sz are the host
 *            loop's float32 values widened; z_sz / x_sz are float32 values after init and float64 from the first step on.
 *   meta     int32 [N][8] = {active, H, W, fill_r, fill_g, fill_b, row, status}.  H, W <= 32768: the slot's frame size;
 *            fill: clip(rint(average colour)); row: the next row of boxes / records this slot writes; status: a bit set that the
 *            kernels only ever OR into - 1: the state is not finite or not below 2^30 in magnitude (or H / W / frame_off out of
 *            range), 2: a computed crop rectangle left its array, 4: row outside [0, rows_cap).
 *   frame_off int64 [N]: byte offset of the slot's current frame, uint8 [H][W][3] RGB, in the one `frames` buffer.
 * Every buffer is device memory.  The arithmetic is the host loop's (vfs_amd/siamfc.py: crop_params, SiamFCProbe._apply_peak) in
 * the types numpy uses there, without fused multiply-adds.  Sizes are checked before any launch: 1 <= N <= 64, 1 <= S <= 8,
 * 1 <= out_size, up <= 4096, r * r <= 1024; non-null buffers; 8-byte aligned fp64 / int64 buffers, 16-byte aligned tap tables
 * and records.
 *
 * vfs_siamfc_batch_crops: for every active slot and scale s the crop of vfs_siamfc_crops with the geometry
 * crop_params((H, W), center, size, out_size, fill) computed on the device in float64, size = x_sz * factors[s], or z_sz when
 * use_z (then S = 1).  factors fp64 [S].  out fp32 [S][N][3][out_size][out_size] - scale-major, so that vfs_xcorr_fwd's
 * `m % nz` pairs slot n's S search maps with exemplar n.  The crop is zeros where crop_and_resize returns zeros, for an inactive
 * slot (nothing else of that slot is read), and for a slot whose state fails the check (status bit 1 or 2; no address is formed
 * from an unchecked state). */
int vfs_siamfc_batch_crops(const uint8_t* frames, const long long* frame_off, const double* state, int* meta, const double* factors,
                           float* out, int N, int S, int out_size, int use_z, vfs_stream_t stream);
/* vfs_siamfc_batch_upsample: vfs_siamfc_upsample (same kernel, same key format) on responses fp32 [S][N][r][r] -> up_out fp32
 * [S][N][up][up], penalty fp32 [S]; scale_max uint64 [N][S]. */
int vfs_siamfc_batch_upsample(const float* responses, const int* tap_idx, const float* tap_w, const float* penalty, float* up_out,
                              unsigned long long* scale_max, int N, int S, int r, int up, vfs_stream_t stream);
/* vfs_siamfc_batch_peak: one workgroup per slot.  For an active slot: {scale_id, row, col} of vfs_siamfc_peak on the slot's S
 * maps of up_in [S][N][up][up]; then SiamFCProbe._apply_peak on the slot's state (total_stride, response_up, instance_sz,
 * scale_lr: the probe's configuration; factors fp64 [S]); boxes[meta.row] (fp64 [rows_cap][4], 1-indexed ltwh computed in float32
 * and widened), records[meta.row] (int32 [rows_cap][4], 16-byte aligned) = {scale_id, row, col, 0}; meta.row += 1.  With
 * meta.row outside [0, rows_cap) nothing is written but status bit 4.  An inactive slot is untouched in every word. */
int vfs_siamfc_batch_peak(const float* up_in, const unsigned long long* scale_max, const double* hann, const double* factors,
                          double* state, int* meta, double* boxes, int* records, long long rows_cap, int N, int S, int up,
                          float one_minus_wi, double window_influence, double total_stride, double response_up, double instance_sz,
                          double scale_lr, vfs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
