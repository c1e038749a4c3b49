// The A/B switchboard of libvfs_hip.so (include/vfs_hip_tuning.h: vfs_set_option): process-global ints that the dispatchers read
// at launch time.  THE list: a new knob is one X(name, default) line here - the declaration below, the definition and the
// name table of vfs_set_option (capi.hip) all come from it.  Every default is the measured-best path.
#pragma once

#define VFS_OPTIONS(X)                                                                                                              \
  /* ---- 3x3 halo-tile kernels (conv_halo.hip, conv_wgrad_halo.hip) */                                                             \
  X(halo, 1)                  /* 1: 3x3 / stride-1 convs use the halo-tile kernels */                                               \
  X(halo_min_fill, 70)        /* percent of a ragged tiling that must be real pixels (100: exact tilings only) */ \
  X(halo_deep_max, 256)       /* the four-stage weight ring (one workgroup per CU) for launches of at most this many workgroups (0: never) */ \
  X(halo_xcd, 1)              /* XCD-aware tile order of the halo kernels (A/B knob) */                                             \
  /* ---- stem (stem.hip) */                                                                                                        \
  X(stem_direct, 1)           /* 1: the direct 7x7 stem kernel; 0: the stem gather of the implicit-GEMM kernel (A/B knob) */        \
  X(stem_blocks, 0)           /* grid cap of the direct stem kernel (0 = default 2048); tests walk many tiles per block */          \
  /* ---- BatchNorm (bn.hip) */                                                                                                     \
  X(bn_ticket, 1)             /* 0: single-workgroup-per-channel-block reduction instead of the chunked ticket reduction */         \
  X(bn_chunk_rows, 64)        /* rows per chunk of the ticket reduction (A/B knob; was 32); values <= 0 are stored as 64 */         \
  X(bn_wide, 1)               /* plain bn_act / bn_bwd_apply on >= 128-channel tensors: whole pixel rows per workgroup (A/B knob) */ \
  X(bn_wide_min_mb, 8)        /* ... from this tensor size (MB) on */                                                               \
  /* ---- implicit-GEMM convolution (conv_igemm.hip, conv_pw.hip) */                                                                \
  X(igemm_bc, 0)              /* 64: force the 64-channel tile (A/B knob) */                                                        \
  X(igemm_xcd, 1)             /* XCD-aware tile order (A/B knob) */                                                                 \
  X(igemm_mfma_stats, 1)      /* forward statistics rows by MFMA from the staged tile (A/B knob; 0: per-element VALU + DPP) */      \
  X(igemm_narrow_below, 513)  /* 64-channel tiles when the 128-channel tiling has fewer tiles than this (0: never); whole-step A/B: R50 9.45 -> 9.32 ms */ \
  X(igemm_onek, 3)            /* single-buffer variant: 0 never, 1 for one-K-step problems (Ktot == 64), 2 every 1x1, 3 always (round 6: default, was 2: the strided / 3x3 gathers too - R18 step 6.85 -> 6.80 ms, R50 7.96 -> 7.93) */ \
  X(igemm_ring_tiles, 512)    /* LDS-DMA ring variant for 1x1 problems with at most this many tiles (0: off) */                     \
  X(igemm_ring_fbn, 1)        /* the DMA ring also for dgrads with fused BatchNorm-backward statistics (A/B knob) */                \
  X(igemm_ring_mfma32, 1)     /* the pure-GEMM DMA ring on 32x32x16 MFMAs with the lean DMA issue (PIPE 5; 0: PIPE 3, A/B knob) */  \
  X(igemm_ring_gather, 0)     /* DMA ring for GATHERED problems (3x3 / strided forward, stride-1 and stride-2 dgrad classes) with at most this many tiles (0: off; measured) */ \
  X(igemm_ring_upfront, 0)    /* ring variant: all fragment reads of a K-step before its MFMAs (measured, no gain) */               \
  X(igemm_ds_quarter, 1)      /* 1x1 / stride-2 / pad-0 dgrad that completes the residual gradient in place (add == dx: the downsample branch of a stage entry): pure GEMM over the quarter grid, no zero planes written or read back (A/B knob; 0: the four parity classes) - same bits */ \
  X(igemm_skinny, 1)         /* skinny GEMM for <= 128-row problems: the head's Linear layers (A/B knob) */                        \
  X(igemm_pw, 0)              /* persistent 1x1 kernel.  0: off (measured slower than the one-tile kernels, MEASUREMENTS.md round 5); 1: where its plan says so; 2: every eligible 1x1 */ \
  X(igemm_pw_min_tiles, 192)  /* igemm_pw = 1: fewer 128-pixel tiles than this leave CUs idle, the split-channel kernels take over */ \
  /* ---- weight gradient (conv_wgrad.hip, conv_wgrad_halo.hip) */                                                                  \
  X(wgrad_lin, 1)             /* the linear-address path for 1x1 / stride-1 problems (A/B knob) */                                  \
  X(wgrad_lin2, 1)            /* ... and its generalisation to evenly tiled 3x3 / stride-2 problems (A/B knob) */                   \
  X(wgrad_ring, 1)            /* the LDS-DMA ring for 1x1 / stride-1 weight gradients with 128 | C, 128 | Cout (0: the register-staged kernel, A/B knob) */ \
  X(wgrad_xcd, 1)             /* XCD-aware block order of the weight-gradient kernels (A/B knob) */                                 \
  /* ---- fp32 evaluation path (exact_f32.hip) */                                                                                   \
  X(conv_f32_variant, 0)      /* A/B knob: 64 / 128 = force that channel tile, 321 = conv_f32_kernel (two barriers per chunk) */    \
  X(conv_f32_dbg, 0)          /* what-if timing (WRONG results): the bits of ConvF32Args::dbg (vfs_ops.h) */                        \
  X(lpx_target, 0)            /* workgroups the key frames of a query tile are split into; 0 = auto: by channel count (A/B knob) */ \
  X(lpx_wgs, 0)               /* workgroups a launch should reach by ALSO splitting a key frame's window; 0 = auto, < 0 = never (note 1) */ \
  X(lpx_minb, 4)              /* ... with at least this many 64-key blocks per workgroup */                                         \
  /* ---- two-pass label propagation (labelprop2.hip) */                                                                            \
  X(lp2, 1)                   /* 0: always the dense kernel (A/B knob) */                                                           \
  X(lp2_dbg, 0)               /* what-if timing (WRONG results): 2 = cache-hot key traffic, 4 = no lists; 16 = list every in-mask candidate (results unchanged: tests read the s~ of the lists) */ \
  X(lp2_fpb, 0)               /* pass 1: key frames per workgroup; 0 = chosen per launch (vfs_lp2_splits) */                        \
  X(lp2_trim, 1)              /* pass 1: windows of masked key frames trimmed to the columns the tile can reach (0: rectangles, A/B knob) */ \
  X(lp2_cap, 0)               /* list entries per (key-frame split, query); 0 = the workspace shared out among the splits in use; 1..15 are stored as 16, < 0 as 0 */ \
  X(lp2_xcd, -1)              /* pass 1 work order: 1 / 2 = XCD-aware (/ staggered), 0 = dispatch order, -1 = by bank width (note 2) */

// note 1, lpx_wgs = 0: 3072 workgroups for C >= 512 (R50 5.33-5.39 vs 5.45-5.50 ms per frame); R18 is faster without the split
//   (1.48 vs 1.54).
// note 2, lp2_xcd = -1: XCD-aware for C = 1024 (ResNet-50: level in time, 2.986 vs 3.004 ms per frame, 4.7 instead of 8.3 GB fetched
//   per launch), dispatch order for narrower banks (ResNet-18, C = 256: 1.015 vs 1.054 ms per frame - short key blocks, the tiles
//   of an XCD wait for the same lines).

#define VFS_OPTION_DECLARE(name, dflt) extern int vfs_option_##name;
VFS_OPTIONS(VFS_OPTION_DECLARE)
#undef VFS_OPTION_DECLARE
