/*
 * rtm3d_hip.h - C ABI of librtm3d_hip.so, the MI355X (gfx950) implementation of the RTM3D
 * inference hot path.
 *
 * The reference (hitfeelee/rtm3d) has no native code and no FFI: its "operator API" for this path
 * is the Python surface  Model.forward / Model.inference / optim_decode_bbox3d.  Each entry point
 * below names the reference interface (file:line under /root/reference) whose arithmetic it
 * replaces; the Python binding a maintainer would add is shown in INTEGRATION.md and is what
 * rtm3d_amd/_lib.py does with ctypes.
 *
 * Conventions
 *   - plain C types only; every pointer named d_* is a DEVICE pointer owned by the caller
 *     (e.g. torch.Tensor.data_ptr()), every h_* pointer is HOST memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are stream-ordered
 *     and never synchronise unless stated;
 *   - every function returns 0 on success, non-zero on error; rtm3d_last_error() then returns a
 *     thread-local description.  "No detections" is not an error (n_out[b] == 0), mirroring the
 *     `None` list entries of models/model.py:33-44;
 *   - a context is not re-entrant: one caller thread at a time, one context per process-GPU (the reference is
 *     single-threaded per process, train_multi_gpu.py:243).  Replays of one context never overlap on the device: calls on
 *     one stream are ordered by the stream, a call on a different stream is ordered behind the previous replay by an event.
 */
#ifndef RTM3D_HIP_H
#define RTM3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTM3D_ABI_VERSION 9
#define RTM3D_MAX_GROUPS 4
#define RTM3D_MAX_TAPS 80

typedef struct rtm3d_ctx rtm3d_ctx;

const char* rtm3d_last_error(void);
int rtm3d_abi_version(void);

/* ------------------------------------------------------------------ context / plan building
 * A context owns the activation workspace (padded NHWC fp16 tensors), the packed + BN-folded
 * weights and an ordered list of kernel launches ("the plan") for ONE network at ONE input shape.
 * The host (Python, rtm3d_amd/plan.py) records the plan once; rtm3d_forward replays it.
 * Replaces: the nn.Module graph walked by Model.forward, models/model.py:20-27.                  */
int rtm3d_ctx_create(int device, rtm3d_ctx** out);
void rtm3d_ctx_destroy(rtm3d_ctx* ctx);

/* Activation tensor: [B][H+2*pad][W+2*pad][C] fp16, zero border (written once at creation and
 * never touched by kernels, which is what implements the convolutions' zero padding).           */
int rtm3d_tensor_create(rtm3d_ctx* ctx, int B, int H, int W, int C, int pad, int* id);
/* Debug / parity helpers: copy channels [c0, c0+C) of the interior to/from fp32 NCHW host memory
 * (synchronous).                                                                                 */
int rtm3d_tensor_download(rtm3d_ctx* ctx, int id, int c0, int C, float* h_nchw);
int rtm3d_tensor_upload(rtm3d_ctx* ctx, int id, int c0, int C, const float* h_nchw);

/* Device blob (packed weights / folded biases).  Copies `bytes` from host; returns blob id.      */
int rtm3d_blob_create(rtm3d_ctx* ctx, const void* h_data, size_t bytes, int* id);
/* Device address and geometry of a plan tensor / device address of a blob: for kernels that fill or read plan storage from
 * outside the replay (rtm3d_gather_peak_patches writes the patch plan's input tensor and its (y, x) blob).  Any output
 * pointer of rtm3d_tensor_info may be NULL.  d_base = padded element [0][0][0][0] (NHWC fp16, border `border`).         */
int rtm3d_tensor_info(rtm3d_ctx* ctx, int id, void** d_base, int* B, int* H, int* W, int* C, int* border);
int rtm3d_blob_address(rtm3d_ctx* ctx, int id, void** d_ptr, size_t* bytes);

/* Copy the caller's fp32 NCHW (B,3,H,W) image into a 4-channel padded NHWC fp16 tensor (4th channel
 * zero, border >= 4): operand layout of the register-direct MFMA stem (kernel = 3 with cin = 4).      */
int rtm3d_op_input_nhwc4(rtm3d_ctx* ctx, int out_tensor);

/* Generic convolution descriptor (one launch; `groups` independent sub-problems on grid.z).
 * Covers conv KxK (any stride / dilation on kernels 0 and 2, and on the per-tile cin = 16 / 32 instances of kernel 3, which
 * index every tap; the rest of kernel 3 is narrower and refuses other taps by name: its vertical-walk instances - stride 1,
 * out_scale 1, cout 16 with cin = 4 or the 6-k-step cin = 16 packing - take only the dense 7x7 / 3x3 taps in row-major
 * order at dilation 1, its cin = 4 instances need the 7 taps of a filter row on adjacent pixels of a 4-channel tensor, and
 * its 16-byte accesses need tensors whose channel count is a multiple of 8), 1x1 over channel slices of wider tensors (the DLA root
 * "concat" never materialises: producers write slices), grouped head convs, and the four
 * sub-pixel phases of ConvTranspose2d(k4,s2,p1) (models/nets/module.py:7-15).
 * Iteration domain: m in [0, B*Hm*Wm) -> (n, y, x).
 *   input  pixel (n, y*in_stride + tap_dy[g][t], x*in_stride + tap_dx[g][t])   (unpadded coords),
 *          channels [in_coff[g] + tap_dc[g][t], ... + cin) of the input tensor (tap_dc = 0 for an ordinary convolution;
 *          a tap may name another channel slice of the same tensor: a DLA block's `project` 1x1 on the pooled map
 *          (models/nets/dla.py:175-198) becomes extra K-steps of the block's second conv instead of a residual, with the
 *          conv's own taps split into 64-channel pseudo-taps so that every tap carries cin = 64 channels)
 *   output pixel (n, y*out_scale + out_oy[g],    x*out_scale + out_ox[g])
 * Epilogue: + bias[cout] (BN folded) [+ residual at the output pixel] [ReLU] -> fp16 NHWC,
 * or (out_nchw_f32 != 0) fp32 NCHW into the caller buffer given to rtm3d_forward.                */
typedef struct rtm3d_conv_desc {
    int in_tensor, out_tensor, res_tensor; /* res_tensor < 0: none; out_tensor < 0 with out_nchw_f32 */
    int Hm, Wm;                            /* iteration domain per image */
    int in_stride, out_scale;
    int cin, cout;                         /* per group (cout = real output channels) */
    int groups, ntaps;
    int in_coff[RTM3D_MAX_GROUPS], out_coff[RTM3D_MAX_GROUPS], res_coff[RTM3D_MAX_GROUPS];
    int out_oy[RTM3D_MAX_GROUPS], out_ox[RTM3D_MAX_GROUPS];
    int tap_dy[RTM3D_MAX_GROUPS][RTM3D_MAX_TAPS], tap_dx[RTM3D_MAX_GROUPS][RTM3D_MAX_TAPS];
    int tap_dc[RTM3D_MAX_GROUPS][RTM3D_MAX_TAPS]; /* channel offset of the tap relative to in_coff (multiple of 8; kernels 0 and 2 only) */
    int s2d_tensor, s2d_coff;              /* s2d_tensor = tensor id + 1, 0 = none (ABI 8; like out_nchw_f32, so that a zero-initialised descriptor asks
                                              for nothing).  Set (kernel 0 or 5, groups 1, out_scale 1, even output height / width): the output is
                                              written a SECOND time in space-to-depth layout - pixel (y, x) to pixel (y >> 1, x >> 1), channels
                                              s2d_coff + ((y & 1) * 2 + (x & 1)) * cout + c of the half-resolution s2d_tensor - so that the neck
                                              can read the feature map from the grid of its transposed conv's input (plan.py: _neck_up_folds).
                                              With out_tensor < 0 (kernel 0) ONLY this copy is written: its readers are rtm3d_op_maxpool_s2d, a
                                              stride-2 conv restated on the copy (stride-1 taps with tap_dc, or kernel 7 with in_s2d) and tap_dc taps. */
    int in_s2d;                            /* kernel 7 only: in_tensor holds the SPACE-TO-DEPTH copy (half resolution, 4 x cin channels at in_coff) of the
                                              map the conv is stated on (Hm, Wm, taps, stride as for the ordinary map) */
    int relu;
    int w_blob, bias_blob;                 /* packed fp16 weights (layout depends on `kernel`), fp32 bias [groups][cout_pad] */
    int kernel;                            /* one of RTM3D_CONV_* below */
    int bn_tile;                           /* MFMA: cout tile the weights were packed for (16/32/64/128) */
    int out_nchw_f32;                      /* 0, or 1..4 = index+1 into rtm3d_forward's out_logits[] */
    int out_H, out_W;                      /* only for out_nchw_f32 */
    int softmax_stat_slot;                 /* -1, or 0..2: the output map is operand u[slot] of the NEXT rtm3d_op_softmax_fuse and this
                                              launch also emits its spatial-softmax partials (per channel max / sum exp over each
                                              128-pixel run) from the epilogue, so the fusion does not re-read the map to reduce it
                                              (keypoint_fpn_fusion.py:67).  Only for kernel = 2 launches that take the halo-tile kernel
                                              (taps within +-1 pixel, stride 1, Hm % 8 == 0, Wm % 32 == 0) with cout = 256 written at
                                              channel offset 0 of a 256-channel tensor; anything else is refused. */
} rtm3d_conv_desc;
/* rtm3d_conv_desc.kernel (1 and 4 are retired and refused) */
#define RTM3D_CONV_MFMA128 0      /* MFMA implicit GEMM, 128-px tile (cin % 64 == 0) */
#define RTM3D_CONV_MFMA256 2      /* MFMA 256x256 tile (cout % 256 == 0) */
#define RTM3D_CONV_SMALLC 3       /* register-direct MFMA (cin 4/16/32) */
#define RTM3D_CONV_C64_HALO 5     /* 64->64 3x3 halo kernel, filter bank in registers (W % 32 == 0, H % 8 == 0) */
#define RTM3D_CONV_C128_HALO 6    /* 3x3 halo kernel for cin, cout % 128 == 0, weights in the bn_tile = 128 packing of RTM3D_CONV_MFMA128
                                     (W % 32 == 0, H % 8 == 0) */
#define RTM3D_CONV_C64S2_HALO 7   /* 64->128 3x3 STRIDE-2 halo kernel, filter bank in registers (output W % 32 == 0, H % 4 == 0; weights fp16
                                     [9 taps][2 k halves][8 tiles][64 lanes][8]) */
int rtm3d_op_conv(rtm3d_ctx* ctx, const rtm3d_conv_desc* desc);

/* DLA-34 stem, fused (models/nets/dla.py:259-279): base_layer 7x7 3->16 + BN + ReLU, level0 3x3 16->16 + BN + ReLU and - when
 * w_l1_blob >= 0 - level1 3x3 stride 2 16->32 + BN + ReLU in ONE launch; the 16-channel full-resolution intermediate maps stay
 * in LDS.  x4_tensor: the NHWC4 image tensor (border >= 4, H % 16 == 0, W % 32 == 0); out_tensor: level0's output (full
 * resolution, 16 channels at out_coff) or level1's (half resolution, 32 channels).  Weights packed as for rtm3d_op_conv
 * kernel = 3 (cin = 4: [7][64][8]; cin = 16: [cout/16][5][64][8]), fp32 biases with BN folded.  Same result as the
 * rtm3d_op_conv launches it replaces up to fp32 summation order.                                                        */
int rtm3d_op_stem_fused(rtm3d_ctx* ctx, int x4_tensor, int out_tensor, int out_coff, int w_base_blob, int b_base_blob,
                        int w_l0_blob, int b_l0_blob, int w_l1_blob, int b_l1_blob);

/* Entry of a DLA level-1 tree with stride 2 on a 32-channel map (DLA-34 level2, models/nets/dla.py:186-206), three reference ops in
 * one launch reading the input once: bottom = max_pool2d(x, 2, 2) (never materialised), proj_tensor = BN(conv1x1(bottom)) (the
 * `project` branch, no ReLU), conv_tensor = ReLU(BN(conv3x3 stride 2 (x))) (tree1.conv1); 32 -> 64 channels each.  Input: 32
 * channels at in_coff of a tensor with border >= 1, H % 16 == 0, W % 64 == 0.  Weights fp16 [9 taps][4][64 lanes][8] and
 * [4][64][8] (MFMA A fragments, K = 32), fp32 biases [64] with BN folded.                                                      */
int rtm3d_op_conv32s2_fused(rtm3d_ctx* ctx, int in_tensor, int in_coff, int conv_tensor, int conv_coff, int proj_tensor, int proj_coff,
                            int w_conv_blob, int b_conv_blob, int w_proj_blob, int b_proj_blob);

/* Tail of a DLA level-1 tree on 64 channels (DLA-34 level2) in one launch, three reference ops reading x1 once and never
 * writing x2: x2 = ReLU(BN(conv3x3(in)) + x1) (tree2's BasicBlock.conv2 + residual, models/nets/dla.py:92-99), out =
 * ReLU(BN(conv1x1(cat[x2, x1]))) (Root.forward, dla.py:233-241) and - when pool_tensor >= 0 - pool = max_pool2d(out, 2, 2)
 * (the next level's `downsample`, dla.py:170-172,190).  in / x1 (res) / out: 64 channels at *_coff of tensors of equal
 * shape, H % 8 == 0, W % 32 == 0, `in` with a border >= 1; pool: 64 channels at half resolution.  w_conv_blob: the
 * kernel = 5 packing of rtm3d_op_conv ([9][2][4][64 lanes][8]); w_root_blob: fp16 [4 output tiles][4 K-steps][64 lanes][8]
 * with lane = fk * 16 + row, element j = root weight [tile * 16 + row][s * 32 + (j >> 2) * 16 + fk * 4 + (j & 3)] over the
 * concatenated input [x2 | x1] (the K order in which the conv's accumulator fragments are handed to the root's MFMAs);
 * fp32 biases [64] with BN folded.  Same result as the rtm3d_op_conv / rtm3d_op_maxpool launches it replaces up to fp32
 * summation order.  out_tensor < 0: the ordinary copy of `out` is not written (needs s2d_tensor).  s2d_tensor >= 0 (a plain tensor id here, -1 = none): `out` is written a second time in space-to-depth layout - pixel (y, x) to half-resolution
 * pixel (y >> 1, x >> 1), channels s2d_coff + ((y & 1) * 2 + (x & 1)) * 64 + c of s2d_tensor - which lets the neck read the
 * feature map at the resolution of the transposed conv's INPUT grid (rtm3d_amd/plan.py: _neck_up_folds).        */
int rtm3d_op_conv64_root(rtm3d_ctx* ctx, int in_tensor, int in_coff, int res_tensor, int res_coff, int conv_relu,
                         int w_conv_blob, int b_conv_blob, int w_root_blob, int b_root_blob,
                         int out_tensor, int out_coff, int root_relu, int pool_tensor, int pool_coff,
                         int s2d_tensor, int s2d_coff);

/* The four final 3x3 convolutions of the heads in one launch (models/nets/header.py:17,27,32,37):
 * input = the nheads x 256-channel tensor written by the grouped head conv (nheads = 4, or 2 for the
 * "smoke" head table), outputs = rtm3d_forward's first nheads fp32 NCHW logit buffers, cout4[i] channels.  Weights: fp16 [head][tap][8 k-blocks][64 lanes][8]
 * (MFMA fragment order, 16 zero-padded rows per head), bias fp32 [head][16].                          */
int rtm3d_op_headout(rtm3d_ctx* ctx, int in_tensor, int w_blob, int bias_blob, int nheads, const int* cout4);
/* Patch plans (peaks-only regression heads, csrc/sparse_heads.hip): `tensor` holds one S x S window per "image" (= detection
 * slot, no border); window position (i, j) of slot s lies at map pixel (y_s + i - origin, x_s + j - origin) with (y_s, x_s)
 * from `yx_blob` ([slots][2] int32, -1 = empty slot; written per batch by rtm3d_gather_peak_patches).  Positions outside
 * the img_H x img_W map are zeroed: they are the zero padding of the next convolution (models/nets/header.py:24-37).  */
int rtm3d_op_patch_mask(rtm3d_ctx* ctx, int tensor, int yx_blob, int img_H, int img_W, int origin);

/* Max pooling k x k / stride / pad over channel slice, NHWC fp16 (models/nets/dla.py:170-172,
 * models/nets/resnet.py:128).  Inputs are post-ReLU (>= 0) so the zero border equals -inf padding. */
int rtm3d_op_maxpool(rtm3d_ctx* ctx, int in_tensor, int in_coff, int out_tensor, int out_coff,
                     int channels, int ksize, int stride, int pad);

/* z_out = z + sum_i u_i * softmax_{H*W}(u_i)  per (image, channel)
 * (models/nets/keypoint_fpn_fusion.py:60-69).  n_u <= 3.                                         */
int rtm3d_op_softmax_fuse(rtm3d_ctx* ctx, int z_in, int z_out, int n_u, const int* u_tensors);

/* 2x2 / stride 2 max-pool (a DLA level's `downsample`, models/nets/dla.py:170-172) of a map that exists only as its space-to-depth
 * copy (rtm3d_conv_desc.s2d_tensor with out_tensor < 0): the window = the four channel slices of one pixel of in_tensor
 * (`channels` each, from in_coff); output: `channels` at out_coff of out_tensor, same resolution as in_tensor.                */
int rtm3d_op_maxpool_s2d(rtm3d_ctx* ctx, int in_tensor, int in_coff, int out_tensor, int out_coff, int channels);

/* Replay the plan.  d_in: fp32 NCHW (B,3,H,W) normalised image batch (detect.py:53), or NULL when the input tensor was
 * filled by rtm3d_preprocess_batch (out_mode 1);
 * d_out_logits[4]: fp32 NCHW (B,3|16|2|2,H/4,W/4) = pred_logits of models/model.py:22-27.        */
int rtm3d_forward(rtm3d_ctx* ctx, void* stream, const float* d_in, float* const d_out_logits[4]);

/* enable != 0: rtm3d_forward replays the plan as ONE hipGraph launch instead of ~60 kernel launches (small batches are
 * launch-gap bound; the reference's detect.py runs bs = 1).  The graph is captured on first use per distinct
 * (d_in, d_out_logits[0..3]) pointer tuple - kernel arguments are baked into it - and up to 8 tuples are cached (LRU).
 * Results are bit-identical to the eager replay.  The live probe (rtm3d_probe_set) forces the eager path.
 * RULE - ALL-KERNEL GRAPHS ONLY: nothing that runs during a replay may be a hipMemset*Async / hipMemcpy*Async (they become
 * memset / memcpy graph NODES).  With three or more graph execs of different node counts alive in one context, re-launching an
 * older exec ran the kernel node behind its memset node with stale arguments (round 3: a conversion pass silently had no effect,
 * a convolution took a memory-access fault; all-kernel graphs alternate correctly), which is why the ticket counters are zeroed
 * by a kernel.  The rule is enforced: after every capture the node types are enumerated (hipGraphGetNodes /
 * hipGraphNodeGetType); a graph with any non-kernel node is destroyed, the context leaves graph mode for good, the call is
 * served by the eager replay and rtm3d_last_error() says why (rtm3d_ctx_graph_stats reports enabled = 0).               */
int rtm3d_ctx_set_graph(rtm3d_ctx* ctx, int enable);
/* TEST HOOK for the rule above: enable != 0 puts one hipMemsetAsync in front of every replay, so that a capture holds a memset
 * node and must be refused (tests/test_gpu_kernels.py::test_graph_with_memset_node_is_refused).  Never set by the product.  */
int rtm3d_ctx_debug_memset_in_replay(rtm3d_ctx* ctx, int enable);
/* DIAGNOSTICS, unsupported: copies n 32-bit words, starting at word `offset`, of the context's debug area to the host (after a
 * device synchronisation).  Only diagnostic builds of the library write there (-DC256_STAMPS: in-kernel s_memtime stamps of the
 * persistent 256 x 256 convolution, tools/gpu_c256_stamps.sh); in the product build the words read zero.                   */
int rtm3d_ctx_debug_read_words(rtm3d_ctx* ctx, int offset, int n, unsigned int* h_out);
/* Graph bookkeeping of a context: captures made, replays served from the cache, whether graph mode is still on (a caller that
 * hands over fresh buffers on every call makes every call a capture; after 32 captures without as many hits the context gives
 * up on graphs - Model.forward_logits(out=...) keeps the addresses stable).  Any pointer may be NULL.                      */
int rtm3d_ctx_graph_stats(rtm3d_ctx* ctx, int* captures, int* hits, int* enabled);

/* Wall time of STAGES of one eager replay: events on the caller's stream in front of the ops mark_ops[0..n_marks) (ascending op
 * indices; n_marks <= 8) and behind the last op; h_ms[i] = mark i -> mark i + 1 (the last: -> end).  (ABI 9: the side-lane replay
 * schedule of ABI 8 - rtm3d_op_schedule / rtm3d_ctx_set_lanes - is gone: measured as no gain for the forward and a slower
 * two-stream pipeline, profiles/r05_neck_lanes.txt.)                                                                        */
int rtm3d_forward_marks(rtm3d_ctx* ctx, void* stream, const float* d_in, float* const d_out_logits[4],
                        int n_marks, const int* mark_ops, float* h_ms);

/* Per-op timing of one replay with hipEvents (synchronous; for profiling/bench):
 * h_ms[i] = elapsed ms of op i; returns number of ops through *n_ops (h_ms may be NULL).          */
int rtm3d_forward_timed(rtm3d_ctx* ctx, void* stream, const float* d_in, float* const d_out_logits[4],
                        float* h_ms, int cap, int* n_ops);
/* Algorithmic work of op i: flops (2*MAC) and minimum bytes moved; name is a static string.       */
int rtm3d_op_info(rtm3d_ctx* ctx, int i, double* flops, double* bytes, const char** name);

/* Live probe for roofline accounting: record a hipEvent pair around op `op_index` on the caller's
 * stream in every rtm3d_forward (op_index < 0 disables); rtm3d_probe_read synchronises on the
 * recorded events and returns the average duration of the (up to 64) most recent launches.          */
int rtm3d_probe_set(rtm3d_ctx* ctx, int op_index);
int rtm3d_probe_read(rtm3d_ctx* ctx, double* avg_ms, int* count);

/* ------------------------------------------------------------------ 2D decode
 * sigmoid -> 3x3 equality NMS -> top-k -> threshold -> gather/regress 8 vertices + 2D box.
 * Replaces Model.inference, models/model.py:29-98,117-132 and nms_hm, utils/model_utils.py:17-26.
 * Inputs fp32 NCHW logits.  Outputs (all device, caller-owned), image b at row b:
 *   d_n[B] int32 count; d_cls[B*topk] int64; d_score[B*topk]; d_mproj[B*topk*2];
 *   d_verts[B*topk*16] (8 x (x,y)); d_bbox[B*topk*4] (x1,y1,x2,y2); rows >= n are untouched.
 * Order within an image: score descending, ties by ascending flat index (class-major).
 * d_workspace: at least rtm3d_decode2d_workspace_bytes(B, ncls, H, W) bytes.
 * Peaks-only mode (d_offset_fr_main == d_main_offset == NULL, used by the "smoke" head table): only
 * d_n, d_cls, d_score and d_mproj = integer key point (x, y) are written.                            */
size_t rtm3d_decode2d_workspace_bytes(int B, int ncls, int H, int W);
int rtm3d_decode2d(void* stream, const float* d_main_kf, const float* d_offset_fr_main,
                   const float* d_main_offset, int B, int ncls, int H, int W, float score_thresh,
                   int topk, float down_sample, void* d_workspace, int32_t* d_n, int64_t* d_cls,
                   float* d_score, float* d_mproj, float* d_verts, float* d_bbox);

/* Peaks-only regression heads: what Model.inference reads of the regression maps is their value at the <= topk peaks
 * (models/model.py:47-50,124-128: offset_fr_main and main_offset through two gathers; vertex_offset is never read).
 * rtm3d_gather_peak_patches: after rtm3d_decode2d in its peaks-only mode, copy for every live slot the samples of the fused
 * map z (padded NHWC fp16, 256 channels, border z_pad) that the three head convolutions of a peak depend on into a
 * 15 x 15 x 256 patch (layout: csrc/sparse_heads.hip) and the peak's (y, x) into d_yx; empty slots get (-1, -1).
 * The caller states the CAPACITY of what is written: d_patch holds patch_slots windows of patch_S x patch_S x 256 halves, d_yx
 * yx_bytes bytes; the call is refused unless patch_S == 15, patch_slots >= B * topk and yx_bytes >= 8 * B * topk.
 * rtm3d_decode2d_finish: sub-pixel key point, 8 vertices and the 2D box of every live slot from the regression logits
 * evaluated at its peak ([B*topk][16] and [B*topk][2] fp32) - the second half of rtm3d_decode2d, same fp32 operation order;
 * d_mproj holds the integer key points on entry and the sub-pixel ones (x down_sample) on return.                      */
int rtm3d_gather_peak_patches(void* stream, const void* d_z, int z_H, int z_W, int z_C, int z_pad, int B, int topk,
                              const int32_t* d_n, const float* d_peak_xy, void* d_patch, int32_t* d_yx,
                              int patch_slots, int patch_S, size_t yx_bytes);
int rtm3d_decode2d_finish(void* stream, int B, int topk, const int32_t* d_n, const float* d_reg_offset_fr_main,
                          const float* d_reg_main_offset, float down_sample, float* d_mproj, float* d_verts, float* d_bbox);

/* ------------------------------------------------------------------ 3D decode
 * Per object: minimise the 8-corner reprojection error over [sin,cos,l,h,w,X,Y,Z] with an fp64
 * L-BFGS-B (m=10, factr=1e7, pgtol=1e-5, maxls=20, unbounded) started at
 * [0,1,l_ref,h_ref,w_ref,ref_loc].  Replaces optim_decode_bbox3d, utils/model_utils.py:264-312
 * (objective :155-177, gradient :206-234) and scipy.optimize.minimize(method='L-BFGS-B').
 * Iteration driver, More'-Thuente line search, BFGS skip rule and stopping tests follow L-BFGS-B 3.0 step by step.
 * `form` selects how the search direction -B^-1 g of the unbounded case is computed (one wavefront per object either way):
 *   RTM3D_SOLVER_PUBLISHED  L-BFGS-B 3.0's published subspace step (formk / subsm / formt) - the arithmetic SciPy runs behind
 *                           utils/model_utils.py:295-296, operation for operation.  THE PRODUCT'S DEFAULT since ABI 9 (the
 *                           Python facade passes it unless told otherwise): on every reference-run fixture all kept boxes
 *                           are within 1e-4 of SciPy's.  Bit-identical to rtm3d_decode3d_reference_form.
 *   RTM3D_SOLVER_DIRECT     the two-loop recursion over the stored pairs - the same vector in exact arithmetic, a third of the
 *                           dependent fp64 operations per iteration (rtm3d_amd/csrc/lbfgsb.h); keep / reject identical, but one
 *                           kept object in ~1000 stops an iteration apart from SciPy (99.1-100 % within 1e-4 per fixture;
 *                           DESIGN.md section 4).  Opt-in.  Bit-identical to rtm3d_decode3d_scalar.
 *   d_cls[N] int64, d_verts[N*16] fp32, d_K[N*9] fp64 (row-major 3x3 per object),
 *   d_dim_ref[ncls*3] fp64 (h,w,l), d_ref_loc[3] fp64.
 * Outputs: d_x[N*8] fp64 final iterate, d_fun[N] fp64, d_nit[N] int32, d_status[N] int32
 * (0 converged, 1 max iterations, 2 abnormal line search, 3 non-finite objective at the start point:
 * NaN / Inf key points give x = x0, fun = NaN, nit = 0 like SciPy does).  The caller applies `fun < 0.1`. */
#define RTM3D_SOLVER_DIRECT 0
#define RTM3D_SOLVER_PUBLISHED 1
int rtm3d_decode3d(void* stream, int N, const int64_t* d_cls, const float* d_verts, const double* d_K,
                   const double* d_dim_ref, int ncls, const double* d_ref_loc, double* d_x,
                   double* d_fun, int32_t* d_nit, int32_t* d_status, int form);

/* Same solver over the fixed-size slots written by rtm3d_decode2d, without a host round trip:
 * slot i = (image i / topk, rank i % topk) is solved iff rank < d_n[image]; other slots get
 * status -1 and are otherwise untouched.  d_K_per_image[B*9].  Outputs have B*topk rows.
 * form: as for rtm3d_decode3d.                                                                                              */
int rtm3d_decode3d_slots(void* stream, int B, int topk, const int32_t* d_n, const int64_t* d_cls,
                         const float* d_verts, const double* d_K_per_image, const double* d_dim_ref, int ncls,
                         const double* d_ref_loc, double* d_x, double* d_fun, int32_t* d_nit, int32_t* d_status, int form);

/* Fixed-size detection records for collecting the results of a sharded batch (new functionality: the reference's
 * inference is single-GPU, detect.py:18): slot (image, rank) -> 32 fp32 =
 *   [0] class  [1] score  [2:4] main key point  [4:20] 8 vertices (x, y)  [20:24] 2D box
 *   [24:27] dimension (h, w, l)  [27:30] location  [30] Ry = atan2(x0, x1)    (the ParamList fields of
 *   utils/model_utils.py:300-303, rounded to fp32)   [31] flag: 0 empty, 1 2D only, 2 3D kept (fun < fun_accept, :298).
 * Slots with rank >= d_n[image] are written as 32 zeros.  d_x/d_fun/d_status (solver outputs of
 * rtm3d_decode3d_slots) may all be NULL: fields 24..30 are then zero and the flag is 0/1.  d_rec: B*topk*32 floats. */
int rtm3d_pack_records(void* stream, int B, int topk, const int32_t* d_n, const int64_t* d_cls, const float* d_score,
                       const float* d_mproj, const float* d_verts, const float* d_bbox, const double* d_x,
                       const double* d_fun, const int32_t* d_status, double fun_accept, float* d_rec);

/* Box post-processing on the device: for every solved slot (d_status >= 0) the eight corners + the centre of the
 * box x = [sin, cos, l, h, w, X, Y, Z] projected through K - calc_proj_corners / create_corners / rotation_matrix,
 * utils/model_utils.py:66-152 - and the bounding rectangle of the eight corners (the 2D box a KITTI label line carries).
 * d_K: topk > 0 -> one K (9 doubles) per image, slot i belongs to image i / topk; topk == 0 -> one K per slot.
 * Outputs: d_proj[N][9][2], d_rect[N][4] = (x1, y1, x2, y2) fp64; unsolved slots get zeros.
 * Non-finite projections (a corner on the plane z + 1e-6 = 0 projects to +-inf, or to NaN where the numerator is 0 too): the
 * rectangle is reduced with IEEE fmin / fmax, where a NaN operand loses - a coordinate is NaN only where all eight corners
 * are, and an infinite corner gives an infinite coordinate.                                                                  */
int rtm3d_project_boxes(void* stream, int N, int topk, const double* d_x, const int32_t* d_status, const double* d_K,
                        double* d_proj, double* d_rect);

/* "smoke" head-table variant (its source is not in the reference snapshot: PARITY
 * UNPINNED, published SMOKE formulation): closed-form box from the 8 regression channels at each key
 * point of the peaks-only decode.  Outputs use the solver's layout x = [sin ry, cos ry, l, h, w, X, Y, Z]. */
int rtm3d_decode_smoke(void* stream, int B, int topk, const int32_t* d_n, const int64_t* d_cls, const float* d_peak_xy,
                       const float* d_reg, int H, int W, float down_sample, const double* d_K_per_image,
                       const double* d_dim_ref, int ncls, double* d_x, double* d_fun, int32_t* d_nit, int32_t* d_status);

/* Input pipeline step in front of the path: letterbox an already resized uint8 HWC
 * image (h x w x 3, channel order as loaded) into the H x W canvas, centred, border = the image's mean
 * colour truncated to uint8 (datasets/dataset_reader.py:175-195), then Normalize/ToTensor/ToNCHW
 * (preprocess/transforms.py:110-120,312-322) -> fp32 CHW at d_out_chw.  d_lut: fp32 [3][256] =
 * float32((v/255. - mean[c]) / std[c]) computed in float64 like the reference; d_sums3: 3 x uint64 scratch. */
int rtm3d_preprocess(void* stream, const uint8_t* d_img_hwc, int h, int w, float* d_out_chw, int H, int W,
                     const float* d_lut, unsigned long long* d_sums3);

/* The same step for a whole batch of ragged images in TWO launches (interior + per-image channel sums, then borders),
 * with the bilinear Resize of the reference's TestTransform in front (preprocess/transforms.py:480-495,
 * cv2.resize INTER_LINEAR: OpenCV's published 11-bit fixed-point algorithm restated - OpenCV is an un-vendored
 * dependency absent from this image, so the resize itself is PARITY UNPINNED; equal source and target sizes are the
 * identity and then the result is bit-identical to rtm3d_preprocess).
 *   h_imgs[B]: HOST array of DEVICE pointers to uint8 HWC images; h_hw[2B] = (h, w) per image;
 *   h_resized_hw[2B] = (h', w') after Resize, or NULL for "already resized";
 *   out_mode 0: d_out = fp32 NCHW (B,3,H,W), the reference's `imgs` (detect.py:53);
 *   out_mode 1: d_out = the network's own operand, fp16 NHWC4 [B][H+2*out_border][W+2*out_border][4] (4th channel 0;
 *               the border itself is not written) - see rtm3d_input_tensor / rtm3d_forward with d_in == NULL;
 *   d_lut fp32 [3][256] as above, d_lut16 the same table rounded to fp16 (mode 1), d_sums: B*3 uint64 scratch. */
int rtm3d_preprocess_batch(void* stream, int B, const uint8_t* const* h_imgs, const int* h_hw, const int* h_resized_hw,
                           void* d_out, int out_mode, int H, int W, int out_border, const float* d_lut, const void* d_lut16,
                           unsigned long long* d_sums);

/* The schedule rtm3d_preprocess_batch gives a batch, from the host-side sizes alone (HOST function, no device access; added
 * without changing any existing declaration).  The batch runs in sub-batches of 64 images; out[(B + 63) / 64] receives one
 * entry per sub-batch - the very numbers the launcher uses, it calls the same function.  An image with a side < 1 or one
 * that does not fit the canvas, and a resized width whose column table does not fit the LDS (rw > 7500), are refused with
 * the launcher's own message.  rtm3d_preprocess_batch validates the WHOLE batch this way (and every image pointer) before
 * its first memset or launch: a refused call has launched nothing.
 * A band of band_rows resized rows is staged in LDS iff its source span fits: (yhi - ylo + 1) * w * 3 + 15 <= stage_bytes
 * (ylo .. yhi: the source rows the band's first and last row interpolate from); otherwise it gathers from global memory.
 * A workgroup takes more than one band when bands > grid_x.                                                          */
typedef struct rtm3d_preprocess_plan {
    int first, count;                      /* images first .. first + count - 1 */
    int col_bytes;                         /* LDS column-coefficient table: widest resized row x 8 B, rounded up to 16 */
    int stage_bytes;                       /* LDS stage of source rows behind it */
    int band_rows;                         /* resized rows per band */
    int bands;                             /* bands of the tallest resized image */
    int grid_x;                            /* interior launch: grid (grid_x, count) x 256 threads, col_bytes + stage_bytes of dynamic LDS */
    int border_grid_x;                     /* border launch: grid (border_grid_x, count) x 256; 0 = every image fills the canvas, no launch */
} rtm3d_preprocess_plan;
int rtm3d_preprocess_batch_plan(int B, const int* h_hw, const int* h_resized_hw, int H, int W, rtm3d_preprocess_plan* out);

/* Device address and geometry of the plan's 4-channel fp16 input tensor (written by rtm3d_op_input_nhwc4 from the caller's
 * fp32 batch, or directly by rtm3d_preprocess_batch in out_mode 1, after which rtm3d_forward is called with d_in == NULL
 * and skips the conversion).  Fails if the plan has no such tensor.                                                  */
int rtm3d_input_tensor(rtm3d_ctx* ctx, void** d_base, int* B, int* H, int* W, int* border);

/* Stream restricted to `n_cus` compute units (hipExtStreamCreateWithCUMask) for the latency-bound
 * 3D decode of the two-stream pipeline; destroy with rtm3d_stream_destroy.                          */
int rtm3d_stream_create_cumask(int device, int n_cus, void** stream);
int rtm3d_stream_destroy(void* stream);

/* Cross-check entries, the arguments of rtm3d_decode3d without `form`, one lane per object (slow; parity tests only):
 *   rtm3d_decode3d_scalar          the direct form: results bit-identical to rtm3d_decode3d(form = RTM3D_SOLVER_DIRECT);
 *   rtm3d_decode3d_reference_form  L-BFGS-B 3.0 with its published subspace step (formk / subsm / formt), the form
 *                                  scipy.optimize.minimize(method='L-BFGS-B') runs (utils/model_utils.py:295-296): bit-identical
 *                                  to rtm3d_decode3d(form = RTM3D_SOLVER_PUBLISHED).                                            */
int rtm3d_decode3d_scalar(void* stream, int N, const int64_t* d_cls, const float* d_verts, const double* d_K,
                          const double* d_dim_ref, int ncls, const double* d_ref_loc, double* d_x,
                          double* d_fun, int32_t* d_nit, int32_t* d_status);
int rtm3d_decode3d_reference_form(void* stream, int N, const int64_t* d_cls, const float* d_verts, const double* d_K,
                                  const double* d_dim_ref, int ncls, const double* d_ref_loc, double* d_x,
                                  double* d_fun, int32_t* d_nit, int32_t* d_status);

/* ------------------------------------------------------------------ fp32 verification executor (regime ii)
 * The product path stores activations and weights in fp16; BASELINE's "3D-box L-inf vs CPU ref" through fp16 logits is
 * bounded by that storage.  These three stateless entry points run the SAME recorded plan
 * (rtm3d_amd/plan.py: tap tables, channel slices, sub-pixel phases, folded BN, composed 1x1 pairs) on padded NHWC *fp32*
 * tensors with fp32 weights and fp64 accumulation, so that Model.forward_logits_fp32 -> rtm3d_decode2d ->
 * rtm3d_decode3d_slots can be compared with the reference's fp32 CPU path (models/model.py:20-27, :29-75,
 * utils/model_utils.py:264-312) to fp32 round-off.  Verification only: simple kernels (no MFMA, no LDS), ~100x slower than
 * rtm3d_forward, never selected by Model.forward.
 * rtm3d_vtensor: channel slice [coff, coff + c) of a padded NHWC fp32 buffer [B][Hp][Wp][C] with border P (zeros), all
 * device memory owned by the caller.                                                                                    */
typedef struct rtm3d_vtensor {
    float* d;
    int Hp, Wp, C, P, coff;
} rtm3d_vtensor;

/* One group of rtm3d_conv_desc (same iteration domain, tap and output-pixel semantics) in fp32.
 * d_w: fp32 [ntaps][cin][cout]; d_bias: fp32 [cout] (BN folded).  cin, in.C and in.coff must be multiples of 4.
 * out_nchw_f32 != 0: out.d is an fp32 NCHW (B, cout, out_H, out_W) buffer (the logits) and out's geometry is ignored.
 * res.d == NULL: no residual.                                                                                           */
typedef struct rtm3d_vconv_desc {
    rtm3d_vtensor in, out, res;
    const float* d_w;
    const float* d_bias;
    int B, Hm, Wm, in_stride, out_scale, out_oy, out_ox;
    int cin, cout, ntaps, relu;
    int out_nchw_f32, out_H, out_W;
    int tap_dy[RTM3D_MAX_TAPS], tap_dx[RTM3D_MAX_TAPS];
} rtm3d_vconv_desc;
int rtm3d_verify_conv_f32(void* stream, const rtm3d_vconv_desc* desc);

/* rtm3d_op_maxpool in fp32 (same zero-border = -inf convention: pooled maps are post-ReLU).                             */
int rtm3d_verify_maxpool_f32(void* stream, const rtm3d_vtensor* in, const rtm3d_vtensor* out, int B, int Ho, int Wo,
                             int channels, int ksize, int stride, int pad);

/* rtm3d_op_softmax_fuse in fp32: z_out = z_in + sum_i u_i * softmax_{H*W}(u_i), operands added in the given order
 * (models/nets/keypoint_fpn_fusion.py:60-69); exp in fp32, the sums in fp64.  u: array of n_u <= 3 tensors;
 * d_workspace: rtm3d_verify_softmax_workspace_bytes(B, C, n_u) bytes.                                                   */
size_t rtm3d_verify_softmax_workspace_bytes(int B, int C, int n_u);
int rtm3d_verify_softmax_fuse_f32(void* stream, const rtm3d_vtensor* z_in, const rtm3d_vtensor* z_out, int n_u,
                                  const rtm3d_vtensor* u, int B, int H, int W, int C, void* d_workspace);

/* ------------------------------------------------------------------ MXFP8 head convolutions (opt-in; csrc/conv_mx8.hip)
 * The Python layer's head_precision='mxfp8' (rtm3d_amd/plan.py): the fused map z is quantised once, the dilation-6 and
 * dilation-1 head convs run on block-scaled e4m3 operands (v_mfma_scale_f32_32x32x64_f8f6f4), the last one writes the fp16
 * tensor rtm3d_op_headout reads.  Added in ABI 9 without changing any existing declaration.
 *
 * MX8 tensor: [B][H+2*pad][W+2*pad][C] OCP e4m3fn bytes and a scale plane [B][H+2*pad][W+2*pad][C/32] of E8M0 bytes
 * (value = e4m3 * 2^(scale - 127)); C % 32 == 0.  The zero border (scale 127) is written once at creation.  MX8 tensor ids
 * are their own namespace: they are accepted only by the functions below.
 * Quantisation (OCP MX v1.0, host restatement: rtm3d_amd/mx8.py): per 32 channels of a pixel shared_exp =
 * floor(log2(amax)) - 8 clamped to [-127, 127] (all-zero block: 127 - i.e. exponent 0), each element round-to-nearest-even
 * e4m3(x / 2^shared_exp) saturated to +-448.                                                                          */
int rtm3d_tensor_create_mx8(rtm3d_ctx* ctx, int B, int H, int W, int C, int pad, int* id);
/* Dequantised fp32 NCHW copy of channels [c0, c0+C) of the interior (synchronous; tests).                              */
int rtm3d_tensor_download_mx8(rtm3d_ctx* ctx, int id, int c0, int C, float* h_nchw);
/* The whole padded arrays, borders included: h_data B*Hp*Wp*C bytes, h_scale B*Hp*Wp*C/32 bytes (synchronous; tests).   */
int rtm3d_tensor_download_mx8_raw(rtm3d_ctx* ctx, int id, void* h_data, void* h_scale);
int rtm3d_tensor_upload_mx8_raw(rtm3d_ctx* ctx, int id, const void* h_data, const void* h_scale);
/* Quantise `channels` (multiple of 32) channels from in_coff (multiple of 8) of an fp16 tensor into out_coff (multiple of
 * 32) of an MX8 tensor of the same B, H, W.  Interior pixels only.                                                      */
int rtm3d_op_quant_mx8(rtm3d_ctx* ctx, int in_tensor, int in_coff, int out_tensor, int out_coff, int channels);
/* Stride-1 convolution over an MX8 input onto a map of the same size: output pixel (n, y, x), channels
 * out_coff[g] + [0, cout) = bias + sum over taps t and channels c of  w[g][co][t][c] * in(n, y + tap_dy[t], x + tap_dx[t],
 * in_coff[g] + c), then ReLU (relu != 0), stored as MX8 (one scale per 32 output channels of a pixel, the rule above) or as
 * fp16 NHWC (out_fp16 = 1, out_tensor is then an ordinary tensor id).  cin % 64 == 0, cout % 256 == 0, in_coff[g] % 64 ==
 * 0, the input tensor's C % 64 == 0; every tap must stay inside the padded input.
 * Blobs, kt = (cin / 64) * ntaps k-steps in the order k = tap * (cin / 64) + chunk:
 *   w_blob      e4m3  [groups][cout / 256][kt][256 rows = output channel % 256][64 = channel chunk * 64 + j]
 *   wscale_blob E8M0  [groups][cout / 256][kt][256 rows][2]   (the scales of channels [0, 32) and [32, 64) of the chunk)
 *   bias_blob   fp32  [groups][cout]  (BN folded)                                                                   */
typedef struct rtm3d_conv_mx8_desc {
    int in_tensor;                     /* MX8 tensor id */
    int out_tensor;                    /* MX8 tensor id, or (out_fp16 = 1) fp16 tensor id */
    int out_fp16;
    int cin, cout, groups, ntaps;      /* per group; groups <= RTM3D_MAX_GROUPS, ntaps <= RTM3D_MAX_TAPS */
    int in_coff[RTM3D_MAX_GROUPS], out_coff[RTM3D_MAX_GROUPS];
    int tap_dy[RTM3D_MAX_TAPS], tap_dx[RTM3D_MAX_TAPS];   /* shared by all groups */
    int relu;
    int w_blob, wscale_blob, bias_blob;
} rtm3d_conv_mx8_desc;
int rtm3d_op_conv_mx8(rtm3d_ctx* ctx, const rtm3d_conv_mx8_desc* desc);

/* ------------------------------------------------------------------ engine files (csrc/engine.cpp; added in ABI 9)
 * An engine file is a realized plan written by rtm3d_amd.engine.save_engine: the state-changing calls the Python plan
 * recorder made (tensor / blob creation and every launch, with the ids the recorder handed out), the packed weights and
 * what a detect step needs.  Loading it replays those calls through the functions above, so a C caller gets the exact
 * launches of the Python path without Python, torch or weight packing.  All integers little-endian.
 *
 *   header (256 bytes, zero-padded):
 *     char magic[8] = "RTM3DENG"; uint32 format_version (RTM3D_ENGINE_FORMAT); uint32 abi_version (RTM3D_ABI_VERSION);
 *     char arch[16] = "gfx950"; char state_digest[64] (hex sha256 of the state dict, rtm3d_amd.weight_cache.state_dict_digest);
 *     uint8 body_sha256[32] (of everything after the header); uint64 body_bytes.
 *     Nothing CU-specific is stored: the runtime picks routes from the context's CU count at replay.
 *   body:
 *     metadata (496 bytes): int32 B, H, W; char backbone[16]; int32 head_precision (0 fp16, 1 mxfp8), header_num_conv,
 *       num_classes, head_channels[4], topk (TOPK_CANDIDATES); float down_sample, score_thresh; int32 n_dim_ref;
 *       double dim_ref[16][3], ref_loc[3]; int32 solver_form (RTM3D_SOLVER_*), use_graph (default of rtm3d_ctx_set_graph);
 *       double fun_accept (0.1)
 *     uint32 n_records, n_blobs; uint64 records_bytes; then the records, each  uint32 opcode, uint32 payload_bytes, payload:
 *        1 tensor_create / 2 tensor_create_mx8   int32 B, H, W, C, pad, id
 *        3 blob_create                           uint64 bytes, offset in the blob area; int32 id, 0
 *       16 op_input_nhwc4 (1 int32)   18 op_stem_fused (9)   19 op_conv32s2_fused (10)   20 op_conv64_root (16)
 *       21 op_headout (in, w, bias, nheads, cout4[4])   22 op_maxpool (8)   23 op_maxpool_s2d (5)
 *       24 op_softmax_fuse (z_in, z_out, n_u, u[3])   25 op_quant_mx8 (5)          (int32 arguments in prototype order)
 *       17 op_conv / 26 op_conv_mx8                 uint32 sizeof(descriptor), then the descriptor bytes
 *     uint64 blob_offset (from the body start, a multiple of 256), blob_bytes; zero padding; the blob area (each blob
 *     at a multiple of 256).
 * `id` is the id the recorder handed out; the loader refuses a replay that gets another one back.  Files of another
 * format or ABI version are refused, not migrated.                                                                      */
#define RTM3D_ENGINE_FORMAT 1
#define RTM3D_ENGINE_MAX_CLASSES 16
typedef struct rtm3d_engine_info {
    int format_version, abi_version;
    char arch[16];
    char state_digest[72];                 /* hex, NUL-terminated */
    int B, H, W;                           /* the input batch: fp32 NCHW (B, 3, H, W) */
    char backbone[16];
    int head_precision, header_num_conv, num_classes;
    int head_channels[4];                  /* channels of the four logit maps (num_classes, 16, 2, 2) */
    int topk;
    float down_sample, score_thresh;
    int n_dim_ref;
    double dim_ref[RTM3D_ENGINE_MAX_CLASSES][3];
    double ref_loc[3];
    int solver_form, use_graph;
    double fun_accept;
    int n_records, n_tensors, n_mx8_tensors, n_blobs, n_launches, reserved;
    uint64_t blob_bytes, file_bytes;
} rtm3d_engine_info;
/* Parse and check a whole engine file on the host, without touching a device: magic, versions, arch, sha256, every length
 * against the end of the file, opcodes against the list above, descriptor sizes, every tensor / blob id against the ones
 * created before it.  On failure rtm3d_last_error() names the record index and the reason.  info may be NULL.          */
int rtm3d_engine_inspect(const char* path, rtm3d_engine_info* info);
/* The same checks, then the device's arch, then a context on `device` into which the records are replayed (with the
 * file's graph default).  On any failure the context is destroyed, *out is NULL and the call returns non-zero.
 * Release with rtm3d_ctx_destroy.                                                                                       */
int rtm3d_engine_load(const char* path, int device, rtm3d_ctx** out, rtm3d_engine_info* info);
/* One detect step of a context made by rtm3d_engine_load, stream-ordered on `stream`, no host synchronisation:
 * rtm3d_forward -> rtm3d_decode2d -> rtm3d_decode3d_slots -> rtm3d_pack_records with the file's metadata.
 * d_in: fp32 NCHW (B, 3, H, W); d_K_per_image: B x 9 fp64; d_rec: B * topk * 32 fp32 records (layout of
 * rtm3d_pack_records); d_workspace: rtm3d_engine_workspace_bytes(ctx) bytes of device memory (logits, decode slots,
 * solver state), owned by the caller.  Keep d_in / d_workspace fixed across calls: a graph replay is keyed by them.    */
size_t rtm3d_engine_workspace_bytes(rtm3d_ctx* ctx);
int rtm3d_engine_detect(rtm3d_ctx* ctx, void* stream, const float* d_in, const double* d_K_per_image, float* d_rec,
                        void* d_workspace);

/* ------------------------------------------------------------------ camera frames (csrc/frames_host.cpp, csrc/frames.hip, csrc/engine.cpp)
 * What lies on either side of a detect step when the caller holds uint8 camera frames and the camera's own intrinsics: the
 * reference's TestTransform bookkeeping (Normalize, Resize, letterbox; preprocess/transforms.py, datasets/dataset_reader.py)
 * and the way back from the pixels of the network canvas to the pixels of the frame.  Added in ABI 9 without changing any
 * existing declaration.
 *
 * HOST helpers (no device access; usable on a machine without a GPU):
 * rtm3d_normalize_luts: h_lut32 [3][256] = float32((v / 255. - mean[c]) / std[c]) evaluated in float64 with float32
 * mean / std (transforms.py:110-120, 312-317), h_lut16 [3][256] = that value rounded to nearest even to IEEE binary16 -
 * the d_lut / d_lut16 operands of rtm3d_preprocess_batch.  Either table may be NULL.
 * rtm3d_frame_geometry: per frame (h, w) = h_hw[2b], h_hw[2b + 1] the size after Resize - resize_to == 0: (h, w);
 * otherwise rate = (double)resize_to / max(h, w), rh = (int)(h * rate), rw = (int)(w * rate) (transforms.py:484-490) - and
 * its centred place on the H x W canvas: pad_w = (W - rw) / 2, pad_h = (H - rh) / 2.  A frame with a side < 1 or one that
 * does not fit the canvas is an error that names the frame.                                                             */
typedef struct rtm3d_frame_geom {
    int h, w;                              /* the camera frame */
    int rh, rw;                            /* after Resize */
    int pad_w, pad_h;                      /* left / top letterbox border on the canvas */
} rtm3d_frame_geom;
int rtm3d_normalize_luts(const float mean[3], const float std[3], float* h_lut32, uint16_t* h_lut16);
int rtm3d_frame_geometry(int B, const int* h_hw, int resize_to, int H, int W, rtm3d_frame_geom* out);

/* Device kernels; h_geom[B] is HOST memory and travels as a kernel argument (no copy, no memset).  All arithmetic is fp64
 * in a fixed operation order, compiled without contraction, so the results are defined bit for bit.  Both entries check the
 * geometry of EVERY frame (h, w, rh, rw >= 1) before the first launch: a refusal names the frame and has changed nothing,
 * whichever frame of the batch it is.
 * rtm3d_frames_adjust_k: d_K_net = the intrinsics of the network canvas from the camera's (both B x 9 fp64): row 0 / w
 * then * rw, row 1 / h then * rh (ToPercentCoords -> Resize -> ToAbsoluteCoords, transforms.py:146-176; the pair is
 * executed for equal sizes too), then cx + pad_w, cy + pad_h (dataset_reader.py:189-193); row 2 is copied.
 * rtm3d_records_to_camera: in place on the B * topk * 32 records of rtm3d_pack_records.  In every slot with flag [31] >= 1
 * the 2D fields - key point [2:4], vertices [4:20], box [20:24] - become
 *   (float)(((double)x - pad_w) * ((double)w / (double)rw)),  (float)(((double)y - pad_h) * ((double)h / (double)rh));
 * [0:2] and [24:32] stay (with consistently adjusted intrinsics the 3D box is the same box); empty slots stay 32 zeros.
 * d_kitti (may be NULL, and then d_K_camera / d_x / d_fun / d_status may be too): B * topk * 16 fp64, one row per slot,
 * all zero unless the slot is kept: the RECORD's flag [31] is 2, and d_status >= 0 and d_fun < fun_accept agree with it.  The
 * flag decides because rtm3d_records_nms3d turns the flag of a suppressed slot 2 -> 1 and leaves the solver outputs alone: a
 * slot it suppressed has no row, whether it ran before this entry or after it (then with its own d_kitti argument).  The row
 * holds the numbers of a KITTI label line (rtm3d_amd/kitti_results.py):
 *   [0] class  [1] alpha = ry - atan2(x, z) wrapped to [-pi, pi)  [2:6] x1 y1 x2 y2 = the bounding rectangle of the eight
 *   corners projected through the CAMERA's intrinsics (the arithmetic of rtm3d_project_boxes), clipped to [0, w - 1] x
 *   [0, h - 1] of the frame  [6:9] h w l  [9:12] x, y + h / 2, z (centre of the bottom face)  [12] ry = atan2(x0, x1)
 *   [13] score  [14] 2  [15] 0.
 *   Non-finite projections: the rectangle is reduced and clipped with IEEE fmin / fmax, where a NaN operand loses - a NaN
 *   coordinate (all eight corners NaN) clips to 0, -inf to 0, +inf to w - 1 / h - 1.
 * d_x / d_fun / d_status: the outputs of rtm3d_decode3d_slots for the same slots.                                         */
int rtm3d_frames_adjust_k(void* stream, int B, const rtm3d_frame_geom* h_geom, const double* d_K_camera, double* d_K_net);
int rtm3d_records_to_camera(void* stream, int B, int topk, const rtm3d_frame_geom* h_geom, float* d_rec,
                            const double* d_K_camera, const double* d_x, const double* d_fun, const int32_t* d_status,
                            double fun_accept, double* d_kitti);

/* One detect step of an engine fed by camera frames, stream-ordered, no host synchronisation:
 * rtm3d_frame_geometry -> rtm3d_preprocess_batch (out_mode 1, into the plan's own input tensor) -> rtm3d_frames_adjust_k ->
 * rtm3d_forward (d_in == NULL) -> rtm3d_decode2d -> rtm3d_decode3d_slots -> rtm3d_pack_records -> rtm3d_records_to_camera.
 * rtm3d_engine_set_frame_params: once per context made by rtm3d_engine_load, before the first frames step: builds both
 * normalisation tables and keeps them on the device.  resize_to: 0 = the frames are fed at their own size, otherwise the
 * longest side after Resize (the reference's INPUT_SIZE).
 * rtm3d_engine_detect_frames: h_imgs[B] HOST array of DEVICE pointers to uint8 (h, w, 3) frames, h_hw[2B] their (h, w);
 * d_K_camera B x 9 fp64, the cameras' own intrinsics; d_rec B * topk * 32 fp32 records in the pixels of each frame;
 * d_kitti NULL or B * topk * 16 fp64 rows (layouts above); d_workspace: rtm3d_engine_frames_workspace_bytes(ctx) bytes =
 * the detect workspace, the channel sums (B x 3 uint64) and the canvas intrinsics.  Keep d_workspace fixed across calls:
 * a graph replay of the forward is keyed by the logit addresses inside it.                                              */
typedef struct rtm3d_frame_params {
    float mean[3], std[3];
    int resize_to;
} rtm3d_frame_params;
int rtm3d_engine_set_frame_params(rtm3d_ctx* ctx, const rtm3d_frame_params* params);
size_t rtm3d_engine_frames_workspace_bytes(rtm3d_ctx* ctx);
int rtm3d_engine_detect_frames(rtm3d_ctx* ctx, void* stream, const uint8_t* const* h_imgs, const int* h_hw,
                               const double* d_K_camera, float* d_rec, double* d_kitti, void* d_workspace);

/* ------------------------------------------------------------------ pixel formats (csrc/frames_convert.hip, csrc/engine.cpp)
 * Camera frames as they reach a GPU - the video decoder's pitched NV12 / P010 surfaces, YUYV / UYVY of UVC and automotive
 * cameras, I420 of software decoders, BGRA or pitched RGB rows of capture APIs - to the tightly packed uint8 (h, w, 3)
 * frames that rtm3d_engine_detect_frames, rtm3d_preprocess_batch and rtm3d_records_draw read.  The conversion is its own
 * launch (one per chunk of 32 frames, descriptors by value, no host synchronisation); the packed copy is what the drawing
 * entry points paint into.  Added in ABI 9 without changing any existing declaration.
 *
 * THE RULE (integers only, int32, >> arithmetic; tests/pixfmt_ref.py restates it in numpy).
 * Chroma of pixel (x, y): 4:2:0 formats (NV12, NV21, I420, P010) use the sample at (x >> 1, y >> 1); 4:2:2 formats (YUYV,
 * UYVY) the chroma of the pixel's own pair on row y.  Nearest-sample replication is deliberate; siting-aware interpolation
 * is out of scope.
 * 8-bit samples: Y' = y - yo with yo = 16 (limited) or 0 (full), U = cb - 128, V = cr - 128, S = 16.
 * P010: sample value = s >> 6 of the little-endian uint16 s; yo = 64 or 0, U = cb - 512, V = cr - 512, S = 18.
 *   R = clamp((cy*Y' + crv*V         + (1 << (S-1))) >> S, 0, 255)
 *   G = clamp((cy*Y' + cgu*U + cgv*V + (1 << (S-1))) >> S, 0, 255)
 *   B = clamp((cy*Y' + cbu*U         + (1 << (S-1))) >> S, 0, 255)
 * The coefficients are round(2^S * v), v the textbook value from (Kr, Kb) = (0.299, 0.114) for BT.601 and (0.2126, 0.0722)
 * for BT.709: cy = sy, crv = 2 (1 - Kr) sc, cbu = 2 (1 - Kb) sc, cgu = -2 Kb (1 - Kb) / Kg sc, cgv = -2 Kr (1 - Kr) / Kg sc
 * with Kg = 1 - Kr - Kb and the scales (sy, sc) = (255/219, 255/224) limited 8-bit, (1, 1) full 8-bit, (255/876, 255/896)
 * limited 10-bit, (255/1023, 255/1023) full 10-bit.  [cy, crv, cgu, cgv, cbu]:
 *   BT.601 limited, 8-bit S = 16 and 10-bit S = 18:  76309, 104597, -25675, -53279, 132201
 *   BT.709 limited, 8-bit S = 16 and 10-bit S = 18:  76309, 117489, -13975, -34925, 138438
 *   BT.601 full, 8-bit:                              65536,  91881, -22553, -46802, 116130
 *   BT.709 full, 8-bit:                              65536, 103206, -12276, -30679, 121609
 *   BT.601 full, 10-bit:                             65344,  91612, -22487, -46664, 115789
 *   BT.709 full, 10-bit:                             65344, 102903, -12240, -30589, 121252
 * (every intermediate is below 1.5e8 in magnitude).  RGB24 / BGR24 / RGBA32 / BGRA32 copy their three colour bytes, GRAY8
 * writes the byte three times; matrix and range are ignored for them.  dst_order 0 writes R G B per pixel, 1 writes B G R -
 * the channel order the checkpoint was trained on, which the library cannot know.
 *
 * REFUSALS, checked for the whole batch before the first launch (the message names the frame; a refused call has launched
 * nothing): an unknown format, matrix or range, reserved != 0; a needed plane or a destination that is NULL; h or w < 1 or
 * > 16384; a pitch below min_pitch; for P010 an odd plane address or an odd pitch.  There is NO other alignment requirement:
 * plane bases, pitches and destinations may be any byte address.  Reads stay inside rows x row bytes of each plane (pitch
 * padding need not exist behind the last row); exactly h * w * 3 bytes are written per frame.                             */
#define RTM3D_PIX_RGB24 0   /* plane 0: R G B per pixel                                  */
#define RTM3D_PIX_BGR24 1
#define RTM3D_PIX_RGBA32 2  /* 4 bytes per pixel, the 4th ignored                         */
#define RTM3D_PIX_BGRA32 3
#define RTM3D_PIX_GRAY8 4   /* R = G = B = the byte (no range mapping)                    */
#define RTM3D_PIX_NV12 5    /* plane 0: Y, w bytes x h rows; plane 1: Cb Cr interleaved, 2*cw bytes x ch rows */
#define RTM3D_PIX_NV21 6    /* the same with Cr Cb                                        */
#define RTM3D_PIX_I420 7    /* plane 0: Y; plane 1: Cb, plane 2: Cr, each cw bytes x ch rows */
#define RTM3D_PIX_YUYV 8    /* plane 0: Y0 Cb Y1 Cr per pixel pair, 4*cw bytes x h rows   */
#define RTM3D_PIX_UYVY 9    /* Cb Y0 Cr Y1                                                */
#define RTM3D_PIX_P010 10   /* NV12 layout with little-endian uint16 samples, value = s >> 6 (10 bits) */
/* cw = (w + 1) / 2, ch = (h + 1) / 2: odd sizes are legal, the last chroma sample serves one pixel / row */
#define RTM3D_YUV_BT601 0
#define RTM3D_YUV_BT709 1
#define RTM3D_YUV_LIMITED 0
#define RTM3D_YUV_FULL 1
typedef struct rtm3d_frame_src {
    const void* plane[3];   /* DEVICE pointers; unused planes NULL */
    int pitch[3];           /* bytes from one row of the plane to the next, >= the row's own bytes */
    int h, w;
    int format, matrix, range, reserved;   /* matrix / range ignored for RGB* and GRAY8; reserved = 0 */
} rtm3d_frame_src;

/* HOST helpers (no device access).
 * rtm3d_frame_src_layout: the planes of a format at a size - their number, the bytes of a row (the least pitch) and the rows
 * of each; entries of unused planes are 0.
 * rtm3d_yuv_coefficients: out[0:5] = the table row [cy, crv, cgu, cgv, cbu] the kernel uses for a YUV format, out[5] = yo,
 * out[6] = the chroma offset (128 or 512), out[7] = S.
 * rtm3d_frames_convert_plan: the schedule rtm3d_frames_convert gives a batch - the very numbers the launcher uses, it calls
 * the same code; out[(B + 31) / 32] receives one entry per chunk.  A frame is cut into runs of px_per_thread pixels of
 * rows_per_thread consecutive rows; thread t = block * threads + lane of grid row i (frame first + i) takes run
 * t % runs_per_row of row group t / runs_per_row, runs_per_row = ceil(w / px_per_thread), and leaves when t >= the frame's
 * own number of runs.  runs is the largest of the chunk, grid_x = ceil(runs / threads), grid_y = count.  The sources are
 * validated as by rtm3d_frames_convert (destinations aside).
 * rtm3d_frames_convert_check: every refusal of rtm3d_frames_convert, without a launch.                                */
int rtm3d_frame_src_layout(int format, int h, int w, int* n_planes, int min_pitch[3], int rows[3]);
int rtm3d_yuv_coefficients(int format, int matrix, int range, int out[8]);
typedef struct rtm3d_convert_plan {
    int first, count;                      /* frames first .. first + count - 1 */
    int px_per_thread, rows_per_thread;    /* 8 pixels of 2 rows (one 4:2:0 chroma row) per thread */
    int threads;                           /* per workgroup */
    int runs;                              /* thread runs of the chunk's largest frame */
    int grid_x, grid_y;
} rtm3d_convert_plan;
int rtm3d_frames_convert_plan(int B, const rtm3d_frame_src* h_src, rtm3d_convert_plan* out);
int rtm3d_frames_convert_check(int B, const rtm3d_frame_src* h_src, uint8_t* const* h_dst, int dst_order);

/* The conversion: h_src[B] and h_dst[B] are HOST arrays, h_dst[b] a DEVICE pointer to h * w * 3 packed bytes.  Stream-ordered. */
int rtm3d_frames_convert(void* stream, int B, const rtm3d_frame_src* h_src, uint8_t* const* h_dst, int dst_order);

/* One detect step of an engine fed by such sources: rtm3d_frames_convert into h_packed[B] (DEVICE buffers of h * w * 3 bytes,
 * which hold the packed frames afterwards - the drawing entry points paint into them), then rtm3d_engine_detect_frames on
 * h_packed with the (h, w) of the sources.  Same workspace, same rtm3d_engine_set_frame_params, stream-ordered with no host
 * synchronisation; sources and frame geometry of the whole batch are validated before the first launch.                 */
int rtm3d_engine_detect_frames_src(rtm3d_ctx* ctx, void* stream, const rtm3d_frame_src* h_src, uint8_t* const* h_packed,
                                   int dst_order, const double* d_K_camera, float* d_rec, double* d_kitti, void* d_workspace);

/* ------------------------------------------------------------------ raw sensor frames (csrc/demosaic.hip, csrc/engine.cpp)
 * GMSL / CSI-2 automotive and machine-vision sensors deliver the colour-filter mosaic itself: one 8 / 10 / 12 / 14 / 16-bit
 * sample per pixel in an RGGB-family Bayer pattern, often MIPI-packed.  This section turns such frames into the tightly packed
 * uint8 (h, w, 3) frames that rtm3d_engine_detect_frames, rtm3d_frames_remap, rtm3d_preprocess_batch and the drawing entry
 * points read: black level, white balance, demosaic, colour matrix and tone table in one launch per chunk of 32 frames,
 * descriptors by value, no host synchronisation.  Added in ABI 9 without changing any existing declaration, struct, plan,
 * engine file or default; a raw frame is NOT an RTM3D_PIX_* format (it needs parameters rtm3d_frame_src has no room for).
 *
 * SAMPLE LAYOUTS (layout, bits).  A frame is one plane, pitch bytes from one row to the next; s(x, y) is the sample value.
 *   RTM3D_RAW_U8       the byte                                                     row bytes w              bits 8
 *   RTM3D_RAW_U16      min(u, 2^bits - 1), u a little-endian uint16                  row bytes 2 w            bits 10 12 14 16
 *   RTM3D_RAW_U16_MSB  u >> (16 - bits)                                              row bytes 2 w            bits 10 12 14 16
 *   RTM3D_RAW_MIPI10   group g = x >> 2 of 5 bytes b0..b4, j = x & 3:
 *                      (b[j] << 2) | ((b4 >> (2 j)) & 3)                             row bytes 5 ceil(w / 4)  bits 10
 *   RTM3D_RAW_MIPI12   group g = x >> 1 of 3 bytes b0..b2, j = x & 1:
 *                      (b[j] << 4) | ((b2 >> (4 j)) & 15)                            row bytes 3 ceil(w / 2)  bits 12
 * The two uint16 layouts need an even plane address and an even pitch; the byte layouts accept any byte address and any pitch
 * at or above the row bytes.  Any w is legal: the last MIPI group of a row is complete in memory.  Reads stay inside h rows
 * of "row bytes" each (pitch padding need not exist behind the last row).
 *
 * PATTERNS.  k = (y & 1) * 2 + (x & 1) is the cell of pixel (x, y); the colours of cells k = 0, 1, 2, 3 are
 *   RTM3D_CFA_RGGB: R G G B    RTM3D_CFA_BGGR: B G G R    RTM3D_CFA_GRBG: G R B G    RTM3D_CFA_GBRG: G B R G.
 *
 * THE RULE (integers only, int32, >> arithmetic; tests/raw_ref.py restates it in numpy).  M = 2^bits - 1.
 * 1. Black level: l = max(s - black[k], 0).
 * 2. White balance on the mosaic: m(x, y) = min((l * gain[k] + 512) >> 10, M); gain is Q10, 1024 is 1.0.
 * 3. Demosaic.  m is read at (fold(x + dx, w), fold(y + dy, h)) with fold(i, n): p = 2 (n - 1), i = i mod p (non-negative),
 *    i >= n gives p - i - reflection without repeating the edge.  p is even, so a folded position has the CFA colour of the
 *    position it stands for; h, w >= 2 is enough.  C = m(x, y); ax1 = the sum of the two horizontal neighbours at distance 1,
 *    ay1 of the two vertical ones, d of the four diagonal ones; ax2, ay2 = the sums of the two neighbours at distance 2 along
 *    each axis.
 *    RTM3D_DEMOSAIC_MHC (Malvar-He-Cutler in sixteenths).  At an R or B pixel - own colour C, the other of R / B called O:
 *      G = (8 C + 4 (ax1 + ay1) - 2 (ax2 + ay2) + 8) >> 4        O = (12 C + 4 d - 3 (ax2 + ay2) + 8) >> 4
 *    At a G pixel - H the colour of its horizontal neighbours, V the colour of its vertical ones:
 *      H = (10 C + 8 ax1 - 2 d - 2 ax2 + ay2 + 8) >> 4           V = (10 C + 8 ay1 - 2 d - 2 ay2 + ax2 + 8) >> 4
 *    Each interpolated value is clamped to [0, M]; the pixel's own colour is C.
 *    RTM3D_DEMOSAIC_BILINEAR:  G = (ax1 + ay1 + 2) >> 2,  O = (d + 2) >> 2,  H = (ax1 + 1) >> 1,  V = (ay1 + 1) >> 1.
 * 4. Colour matrix, Q10, signed, row-major:  c_i = clamp((ccm[3i] R + ccm[3i+1] G + ccm[3i+2] B + 512) >> 10, 0, M).
 *    The identity (1024 on the diagonal) gives (R, G, B) back.
 * 5. Tone: t = c >> (bits - 12) when bits >= 12, else c << (12 - bits); the byte is d_tone[t], d_tone a table of 4096 bytes
 *    on the device and plain data (any byte address); with d_tone == NULL the byte is t >> 4.
 * 6. The three bytes are written R G B (dst_order 0) or B G R (1).  Exactly h * w * 3 bytes are written per frame; the
 *    destination may be any byte address.
 * With the bounds below every intermediate stays below 2^31 (65535 * 16384 + 512 and 3 * 65535 * 8192 + 512).
 *
 * REFUSALS, checked for the whole batch before the first launch (the message names the frame; a refused call has launched
 * nothing): an unknown layout, pattern, method or dst_order; bits not legal for the layout; reserved or pad != 0; a NULL plane
 * or destination; h or w < 2 or > 16384; a pitch below the row bytes; for a uint16 layout an odd address or an odd pitch;
 * black[k] > M; gain[k] > 16384; |ccm[i]| > 8192.
 *
 * OUT OF SCOPE: auto white balance and exposure, lens shading, defect pixels, denoising; decompanding of piecewise-linear HDR
 * sensors (the tone table acts after the demosaic); RCCB, RCCC, quad-Bayer, X-Trans; fusing the demosaic into the lens remap
 * or the preprocess; parity with OpenCV's cvtColor of COLOR_Bayer* - the rule restates the published filters, OpenCV was not
 * at hand to pin them against (as with the lens and evaluation restatements).                                            */
#define RTM3D_RAW_U8 0
#define RTM3D_RAW_U16 1
#define RTM3D_RAW_U16_MSB 2
#define RTM3D_RAW_MIPI10 3
#define RTM3D_RAW_MIPI12 4
#define RTM3D_CFA_RGGB 0
#define RTM3D_CFA_BGGR 1
#define RTM3D_CFA_GRBG 2
#define RTM3D_CFA_GBRG 3
#define RTM3D_DEMOSAIC_MHC 0
#define RTM3D_DEMOSAIC_BILINEAR 1
typedef struct rtm3d_raw_src {             /* 80 bytes */
    const void* plane;                     /* DEVICE */
    const uint8_t* d_tone;                 /* DEVICE, 4096 bytes, or NULL */
    int pitch, h, w;
    int layout, bits, pattern, reserved;   /* reserved = 0 */
    uint16_t black[4], gain[4];            /* per cell k */
    int16_t ccm[9], pad;                   /* pad = 0 */
} rtm3d_raw_src;

/* HOST helpers (no device access).
 * rtm3d_raw_src_layout: the bytes of a row (the least pitch) and the rows of the plane of a layout at a size.
 * rtm3d_frames_demosaic_plan: the schedule rtm3d_frames_demosaic gives a batch - the very numbers the launcher uses, it calls
 * the same code; out[(B + 31) / 32] receives one entry per chunk.  A frame is cut into tiles of tile_w x tile_h pixels; a
 * workgroup of `threads` stages its tile with `halo` more samples on every side (after steps 1-2, folded) and then every
 * thread writes 8 pixels of 2 consecutive rows.  Workgroup t of grid row i (frame first + i) takes tile t % tiles_x of tile
 * row t / tiles_x, tiles_x = ceil(w / tile_w), and leaves when t >= the frame's own number of tiles.  tiles is the largest of
 * the chunk, grid_x = tiles, grid_y = count.  The sources are validated as by rtm3d_frames_demosaic (destinations aside).
 * rtm3d_frames_demosaic_check: every refusal of rtm3d_frames_demosaic, without a launch.                                */
int rtm3d_raw_src_layout(int layout, int bits, int h, int w, int* min_pitch, int* rows);
typedef struct rtm3d_demosaic_plan {
    int first, count;                      /* frames first .. first + count - 1 */
    int tile_w, tile_h, halo;              /* 128 x 32 pixels, 2 samples around them (both methods) */
    int threads;                           /* per workgroup */
    int tiles;                             /* tiles of the chunk's largest frame */
    int grid_x, grid_y;
} rtm3d_demosaic_plan;
int rtm3d_frames_demosaic_plan(int B, const rtm3d_raw_src* h_src, int method, rtm3d_demosaic_plan* out);
int rtm3d_frames_demosaic_check(int B, const rtm3d_raw_src* h_src, uint8_t* const* h_dst, int method, int dst_order);

/* The demosaic: h_src[B] and h_dst[B] are HOST arrays, h_dst[b] a DEVICE pointer to h * w * 3 packed bytes.  Frames of
 * different sizes, layouts and patterns may share a chunk.  Stream-ordered.                                              */
int rtm3d_frames_demosaic(void* stream, int B, const rtm3d_raw_src* h_src, uint8_t* const* h_dst, int method, int dst_order);

/* One detect step of an engine fed by raw sensor frames, the twin of rtm3d_engine_detect_frames_src: rtm3d_frames_demosaic
 * into h_packed[B] (DEVICE buffers of h * w * 3 bytes, which hold the packed frames afterwards), then
 * rtm3d_engine_detect_frames on h_packed with the (h, w) of the sources.  Same workspace, same rtm3d_engine_set_frame_params,
 * stream-ordered with no host synchronisation; everything either step would refuse is refused before the first launch.   */
int rtm3d_engine_detect_frames_raw(rtm3d_ctx* ctx, void* stream, const rtm3d_raw_src* h_src, uint8_t* const* h_packed,
                                   int method, int dst_order, const double* d_K_camera, float* d_rec, double* d_kitti,
                                   void* d_workspace);

/* ------------------------------------------------------------------ JPEG frames (csrc/jpeg_host.cpp, csrc/jpeg.hip, csrc/engine.cpp)
 * USB and IP cameras deliver MJPEG and recorded driving sets ship JPEG files.  This section turns baseline JPEG byte streams
 * into the tightly packed uint8 (h, w, 3) frames every other entry point reads.  The work splits where the format splits: the
 * Huffman decoding is serial per stream and stays on the HOST, threaded over the frames of a batch; dequantisation, the 8 x 8
 * inverse DCT, chroma upsampling and YCbCr -> RGB - all the arithmetic and all the pixel traffic - run on the DEVICE, one
 * launch per chunk of 32 frames, descriptors by value, no host synchronisation.  Added in ABI 9 without changing any existing
 * declaration, struct, plan, engine file or default.  The rule is libjpeg's default decode (the `islow` inverse DCT, "fancy"
 * upsampling, its fixed-point colour tables), bit for bit: tests/jpeg_ref.py restates it in numpy and tests/golden/jpeg_cases.npz
 * pins it against libjpeg-turbo's pixels.  (One stated difference: libjpeg replicates a subsampled chroma plane of at most 2
 * samples in width instead of interpolating it - 4:2:2 and 4:2:0 frames up to 4 pixels wide - while this rule interpolates at
 * every width; measured against libjpeg-turbo, frames 5 pixels wide and wider agree, narrower subsampled ones need not.)
 *
 * ACCEPTED STREAMS: SOI ... EOI with one frame; SOF0, or SOF1 with Huffman coding; sample precision 8; ONE interleaved scan of
 * all components with Ss = 0, Se = 63, Ah = Al = 0.  1 component (grey; any sampling factors, decoded as 1 x 1), or 3 components
 * taken as Y Cb Cr with chroma sampling 1 x 1 and luma sampling (H, V) = (1, 1) 4:4:4, (2, 1) 4:2:2 or (2, 2) 4:2:0.  DQT with 8-
 * or 16-bit entries; DHT anywhere before SOS, a later definition replaces an earlier one; a Huffman table 0 or 1 the stream
 * never defines is the table of ITU-T T.81 Annex K (K.3 / K.5 for id 0, K.4 / K.6 for id 1), as MJPEG cameras rely on.  DRI /
 * RSTn with any interval; fill bytes (0xFF) before markers; APPn and COM are skipped, except that an Adobe APP14 segment with
 * transform 0 is refused.  Bytes after EOI are ignored; a missing EOI after a complete scan is accepted.
 * REFUSED, each with a message that names the reason (and, through the batch entry points, the frame; a refused call has
 * launched nothing): progressive (SOF2), lossless, hierarchical or arithmetic coding; 12-bit precision; 2 or 4 components; any
 * other sampling, 1 x 2 included; several scans; a quantisation table that was never defined, a Huffman table 2 or 3 that was
 * never defined; a Huffman code that is not in its table; a run that passes coefficient 63; entropy-coded data that ends before
 * the last MCU; a restart marker that is missing or out of sequence; h or w of 0 or above 16384; a segment length that runs
 * past the end of the buffer.
 *
 * THE COEFFICIENT BUFFER of a frame (int16, what rtm3d_jpeg_entropy_decode writes and the device stage reads):
 *   [0, 192)      three quantisation tables of 64 uint16 in natural order k = 8 v + u, table c that of component c (zero when
 *                 the frame has no such component);
 *   then the planes Y, Cb, Cr (grey: Y alone).  The block grid of component c is padded to whole MCUs: bw_c = mcus_x * H_c,
 *   bh_c = mcus_y * V_c with mcus_x = ceil(w / (8 Hmax)), mcus_y = ceil(h / (8 Vmax)).  Block (bx, by) starts at
 *   (by * bw_c + bx) * 64 of its plane and holds its 64 coefficients in natural order.  Every offset is a multiple of 64.
 *   Values are the decoded integers - DC after prediction, the predictor reset at every restart - stored with two's-complement
 *   wrap.  mode: RTM3D_JPEG_GREY, _444, _422, _420; (h, w, mode) determine the whole layout.
 *
 * THE RULE (int32 with two's-complement wrap, >> arithmetic; on a stream an encoder produced nothing wraps).
 * 1. Dequantise: d[k] = c[k] * q[k].
 * 2. Inverse DCT.  The one-dimensional pass on x0..x7 with shift s (constants: round(x * 8192) of libjpeg's jidctint):
 *      z1 = (x2 + x6) * 4433;  t2 = z1 - x6 * 15137;  t3 = z1 + x2 * 6270;  t0 = (x0 + x4) << 13;  t1 = (x0 - x4) << 13;
 *      t10 = t0 + t3;  t13 = t0 - t3;  t11 = t1 + t2;  t12 = t1 - t2;
 *      a0 = x7, a1 = x5, a2 = x3, a3 = x1;  z1 = a0 + a3;  z2 = a1 + a2;  z3 = a0 + a2;  z4 = a1 + a3;  z5 = (z3 + z4) * 9633;
 *      a0 *= 2446;  a1 *= 16819;  a2 *= 25172;  a3 *= 12299;  z1 *= -7373;  z2 *= -20995;
 *      z3 = z3 * -16069 + z5;  z4 = z4 * -3196 + z5;  a0 += z1 + z3;  a1 += z2 + z4;  a2 += z2 + z3;  a3 += z1 + z4;
 *      outputs 0..7 = t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3, each (v + 2^(s-1)) >> s.
 *    Pass 1 runs down every column with s = 11, pass 2 along every row of the result with s = 18; the sample is
 *    clamp(v + 128, 0, 255).
 * 3. Each component plane is cut to its real size cw = ceil(w * H_c / Hmax), ch = ceil(h * V_c / Vmax); the chroma of 4:2:2 and
 *    4:2:0 is upsampled with neighbour indices clamped into that real size (never into the MCU padding):
 *      4:2:2   o[2i] = (3 p[i] + p[i-1] + 1) >> 2,  o[2i+1] = (3 p[i] + p[i+1] + 2) >> 2;
 *      4:2:0   output row 2j + k: s[i] = 3 p[j][i] + p[j-1][i] for k = 0, 3 p[j][i] + p[j+1][i] for k = 1; then
 *              o[2i] = (3 s[i] + s[i-1] + 8) >> 4,  o[2i+1] = (3 s[i] + s[i+1] + 7) >> 4.
 * 4. Colour: R = y + ((91881 (cr - 128) + 32768) >> 16),  B = y + ((116130 (cb - 128) + 32768) >> 16),
 *    G = y + ((-22554 (cb - 128) - 46802 (cr - 128) + 32768) >> 16), each clamped to [0, 255]; grey writes y three times.
 * 5. The three bytes are written R G B (dst_order 0) or B G R (1).  Exactly h * w * 3 bytes are written per frame; the
 *    destination may be any byte address.
 *
 * OUT OF SCOPE: entropy decoding on the device (one lane per restart interval included); progressive, arithmetic, 12-bit, CMYK /
 * YCCK and 1 x 2 sampling; tolerant decoding of damaged streams (libjpeg paints the missing part grey; here the stream is
 * refused); EXIF orientation, ICC profiles, PNG; decoding straight into the network input or through the lens map; skipping
 * all-zero blocks by a per-block end index.  (Encoding: the section "JPEG encoding" below.)                               */
#define RTM3D_JPEG_GREY 0
#define RTM3D_JPEG_444 1
#define RTM3D_JPEG_422 2
#define RTM3D_JPEG_420 3
typedef struct rtm3d_jpeg_stream_info {
    int h, w, components, mode;            /* mode: RTM3D_JPEG_* */
    int restart_interval;                  /* MCUs, 0 = none */
    int mcus_x, mcus_y;
    int bw[3], bh[3];                      /* block grid of each component (0 for a component the frame lacks) */
    int reserved;
    size_t table_offset[3];                /* 0, 64, 128 */
    size_t plane_offset[3];                /* in int16, from the start of the buffer */
    size_t coef_count;                     /* int16 of the whole buffer, a multiple of 64 */
} rtm3d_jpeg_stream_info;

/* HOST functions (csrc/jpeg_host.cpp; no device access, safe to call from several threads at once).
 * rtm3d_jpeg_info: parses the headers up to and including SOS, makes every refusal that needs no entropy decoding.
 * rtm3d_jpeg_entropy_decode: the same, then Huffman-decodes the scan (8 bits of lookahead per table step) into
 * h_coef[0 .. coef_count) in the layout above; refused when capacity (in int16) is below coef_count.  Whatever the bytes
 * are, nothing outside data[0 .. bytes) is read and nothing outside h_coef[0 .. capacity) is written.
 * rtm3d_jpeg_workspace_bytes: the bytes of the staging buffer and of the device coefficient buffer of rtm3d_frames_jpeg for
 * these B streams - the sum of their coef_count * 2.                                                                     */
int rtm3d_jpeg_info(const uint8_t* data, size_t bytes, rtm3d_jpeg_stream_info* out);
int rtm3d_jpeg_entropy_decode(const uint8_t* data, size_t bytes, int16_t* h_coef, size_t capacity);
int rtm3d_jpeg_workspace_bytes(int B, const uint8_t* const* h_data, const size_t* h_bytes, size_t* bytes);

/* The device stage alone (csrc/jpeg.hip): steps 1-5 for B frames whose coefficient buffers are on the device.  h_frames[B]
 * and h_dst[B] are HOST arrays; d_coef a DEVICE pointer, 16-byte aligned, to the frame's buffer; h_dst[b] a DEVICE pointer
 * to h * w * 3 bytes.  Frames of different sizes and modes may share a chunk.  Stream-ordered, no host synchronisation.
 * rtm3d_frames_jpeg_plan: the schedule of a batch, the very numbers the launcher uses; out[(B + 31) / 32] receives one
 * entry per chunk.  A frame is cut into tiles of tile_w x tile_h pixels.  A workgroup of `threads` first runs the inverse DCT
 * of every block under its tile, one block per thread and step, into LDS - for subsampled chroma also the blocks that hold
 * the `halo` chroma samples beyond each tile edge, which are computed again by the neighbouring tile - and then every thread
 * writes 8 pixels of 4 consecutive rows.  Workgroup t of grid row i (frame first + i) takes tile t % tiles_x of tile row
 * t / tiles_x, tiles_x = ceil(w / tile_w), and leaves when t >= the frame's own number of tiles.  tiles is the largest of the
 * chunk, grid_x = tiles, grid_y = count.
 * rtm3d_frames_jpeg_check: every refusal of rtm3d_frames_jpeg_idct, without a launch: B < 1, a NULL array, coefficient
 * buffer or destination, a buffer that is not 16-byte aligned, an unknown mode or dst_order, reserved != 0, h or w outside
 * 1..16384.  The message names the frame.                                                                                */
typedef struct rtm3d_jpeg_frame {
    const int16_t* d_coef;                 /* DEVICE */
    int h, w, mode, reserved;              /* reserved = 0 */
} rtm3d_jpeg_frame;
typedef struct rtm3d_jpeg_plan {
    int first, count;                      /* frames first .. first + count - 1 */
    int tile_w, tile_h, halo;              /* 128 x 64 pixels; 1 chroma sample beyond each edge */
    int threads;                           /* per workgroup */
    int tiles;                             /* tiles of the chunk's largest frame */
    int grid_x, grid_y;
} rtm3d_jpeg_plan;
int rtm3d_frames_jpeg_plan(int B, const rtm3d_jpeg_frame* h_frames, rtm3d_jpeg_plan* out);
int rtm3d_frames_jpeg_check(int B, const rtm3d_jpeg_frame* h_frames, uint8_t* const* h_dst, int dst_order);
int rtm3d_frames_jpeg_idct(void* stream, int B, const rtm3d_jpeg_frame* h_frames, uint8_t* const* h_dst, int dst_order);

/* The chain: B streams h_data[b][0 .. h_bytes[b]) on the host to B packed frames on the device.
 *   1. rtm3d_jpeg_info on every stream;  2. every refusal that needs no decoding, for the whole batch: a stream's own, a
 *   destination of fewer than h * w * 3 bytes (h_dst_bytes[b]), a capacity below rtm3d_jpeg_workspace_bytes;
 *   3. the entropy decode of the B streams into h_stage, frame after frame, on n_threads host threads (0: min(B, 8); at most
 *   64), each stream refused as in "REFUSED";  4. one hipMemcpyAsync per chunk of 32 frames from h_stage to the same offset
 *   of d_coef;  5. rtm3d_frames_jpeg_idct.
 * Nothing is launched or copied unless every stream decoded.  h_stage is caller-owned HOST memory of `capacity` bytes -
 * pinned, or the copies are not asynchronous - and d_coef a DEVICE buffer of as many, 128-byte aligned.  The call returns
 * when the decode is done and the rest is queued: h_stage may be reused once the copies have completed on the stream (an
 * event recorded behind the call), d_coef once the kernels have.                                                         */
int rtm3d_frames_jpeg(void* stream, int B, const uint8_t* const* h_data, const size_t* h_bytes, int16_t* h_stage, int16_t* d_coef,
                      size_t capacity, uint8_t* const* h_dst, const size_t* h_dst_bytes, int dst_order, int n_threads);

/* One detect step of an engine fed by JPEG streams, the twin of rtm3d_engine_detect_frames_raw: rtm3d_frames_jpeg into
 * h_packed[B] (DEVICE buffers of h_packed_bytes[b] >= h * w * 3 bytes, which hold the packed frames afterwards), then
 * rtm3d_engine_detect_frames on h_packed with the (h, w) of the streams.  Same workspace, same rtm3d_engine_set_frame_params;
 * everything either step would refuse is refused before the first launch.                                                */
int rtm3d_engine_detect_frames_jpeg(rtm3d_ctx* ctx, void* stream, const uint8_t* const* h_data, const size_t* h_bytes,
                                    int16_t* h_stage, int16_t* d_coef, size_t capacity, uint8_t* const* h_packed,
                                    const size_t* h_packed_bytes, int dst_order, int n_threads, const double* d_K_camera, float* d_rec,
                                    double* d_kitti, void* d_workspace);

/* ------------------------------------------------------------------ JPEG encoding (csrc/jpeg_enc.hip, csrc/jpeg_host.cpp)
 * The way back out: painted frames and bird's-eye panels (or any packed frame) become baseline JPEG streams - MJPEG, .jpg
 * files - with no image library.  The mirror image of "JPEG frames", with the same split and the same coefficient buffer:
 * colour conversion, edge replication, chroma downsampling, the 8 x 8 forward DCT and the quantisation - all the arithmetic
 * and all the pixel traffic - run on the DEVICE, one launch per chunk of 32 frames, descriptors and tables by value, no host
 * synchronisation; the Huffman coding is serial per stream and stays on the HOST, threaded over the frames of a batch.  Added
 * in ABI 9 without changing any existing declaration, struct, plan, engine file or default.  The rule is libjpeg's default
 * encode (jccolor, h2v1 / h2v2 downsampling without smoothing, the `islow` forward DCT, the Annex K Huffman tables, its
 * marker layout), byte for byte: tests/jpeg_enc_ref.py restates it in numpy and tests/golden/jpeg_encode_cases.npz pins it
 * against the streams libjpeg-turbo wrote (Huffman tables not optimised).
 *
 * THE RULE (int32, >> arithmetic).  Input: a packed uint8 (h, w, 3) frame at any byte address, bytes R G B (src_order 0) or
 * B G R (1); 1 <= h, w <= 16384; mode RTM3D_JPEG_GREY / _444 / _422 / _420.
 * 1. Colour:  Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *             Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
 *             Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16
 *    Grey keeps Y alone; R = G = B = v gives Y = v exactly.
 * 2. Edges, in libjpeg's order (it matters for the last chroma row).  For component c with luma sampling (H, V), in the
 *    decoder's layout: cw = ceil(w H_c / H), ch = ceil(h V_c / V), wib = ceil(cw / 8), hib = ceil(ch / 8) - the REAL block grid.
 *    Full-resolution columns are replicated from column w - 1 out to wib * 8 * (H / H_c); full-resolution rows from row h - 1
 *    up to a multiple of V; then the plane is downsampled; then the downsampled rows are replicated from row ch - 1 up to
 *    hib * 8.
 * 3. Downsampling of chroma:  4:2:2  o[i] = (p[2i] + p[2i+1] + b) >> 1, b = 0, 1, 0, 1 ... by i;
 *    4:2:0  o[j][i] = (p[2j][2i] + p[2j][2i+1] + p[2j+1][2i] + p[2j+1][2i+1] + b) >> 2, b = 1, 2, 1, 2 ... by i.
 * 4. Forward DCT on samples - 128 (libjpeg's jfdctint: CONST_BITS 13, PASS1_BITS 2; the eight constants of the inverse rule).
 *    The one-dimensional pass on d0..d7:
 *      t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
 *      t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
 *      o0 = (t10 + t11) << 2, o4 = (t10 - t11) << 2 in pass 1; (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2 in pass 2;
 *      z1 = (t12 + t13) * 4433;  o2 = D(z1 + t13 * 6270);  o6 = D(z1 - t12 * 15137);
 *      z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) * 9633;
 *      t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;  z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
 *      o7 = D(t4 + z1 + z3), o5 = D(t5 + z2 + z4), o3 = D(t6 + z2 + z3), o1 = D(t7 + z1 + z4);
 *    D(x) = (x + 2^(s-1)) >> s.  Pass 1 runs along every row with s = 11, pass 2 down every column of the result with s = 15.
 * 5. Quantisation: a = (|c| + 4 q[k]) / (8 q[k]), truncating; the coefficient is c < 0 ? -a : a; q in natural order, 1..255.
 *    (The device divides by one multiplication, csrc/jpeg_quant.h, proven over every q and every |c| <= 32767.)
 * 6. Tables: rtm3d_jpeg_quality_tables(quality 1..100): scale = quality < 50 ? 5000 / quality : 200 - 2 quality,
 *    t[k] = clamp((base[k] * scale + 50) / 100, 1, 255), base the luminance / chrominance table of Annex K (K.1 / K.2).  A
 *    caller may pass any two tables of 1..255 instead.  Y uses the first, Cb and Cr the second.
 * 7. Entropy coding (host).  Blocks in the decoder's MCU order; the Huffman tables of Annex K (K.3 / K.5 for Y, K.4 / K.6 for
 *    chroma; grey writes DC 0 / AC 0 only); one DC predictor per component, reset at every restart; a block outside its
 *    component's wib x hib grid is coded as DC difference 0 and end of block without reading the buffer (what libjpeg's dummy
 *    blocks come to); ZRL for every 16 zeros in front of a coefficient, EOB for a zero tail; 0xFF is followed by a stuffed
 *    0x00; the last byte before every RSTn and before EOI is padded with 1-bits; RSTn after every `restart` MCUs (0: none).
 *    Layout: SOI, APP0 (JFIF 1.01, units 0, density 1 x 1, no thumbnail), DQT table 0, [DQT table 1], SOF0 (components 1, 2, 3),
 *    DHT DC 0, DHT AC 0, [DHT DC 1, DHT AC 1], [DRI], SOS, data, EOI - the bracketed tables for colour, DRI when restart > 0.
 *
 * THE COEFFICIENT BUFFER is the decoder's, exactly ("JPEG frames").  The device stage writes the three tables (zero for a
 * component the frame lacks), every real block, and ZEROS into the padding blocks of the grid: the whole buffer is defined,
 * rtm3d_frames_jpeg_idct can read it, and rtm3d_jpeg_entropy_decode of an encoded stream equals it on every real block.
 *
 * THE SIZE BOUND (rtm3d_jpeg_encode_bound).  Headers: 2 + 18 + 69 t + (10 + 3 n) + 216 t + [6] + (8 + 2 n) bytes for n
 * components and t = 1 (grey) or 2 tables.  A block: the DC symbol is at most 11 code bits + 11 value bits; every Huffman
 * symbol behind it can be charged to coefficients of its own - a coefficient's symbol (at most 16 code + 10 value bits) to that
 * coefficient, a ZRL (at most 16 bits) to the 16 zeros it stands for, the EOB to the zero tail - so no coefficient carries
 * more than 26 bits and a block no more than 22 + 63 * 26 = 1660 bits = 207.5 bytes.  k blocks between two markers end on a
 * byte boundary after at most ceil(207.5 k) <= 208 k bytes, and stuffing at most doubles them: 416 bytes per coded block
 * (padding blocks included), 2 per restart marker, 2 for EOI.  The bound is the sum.
 *
 * OUT OF SCOPE: optimised Huffman tables, progressive coding, trellis quantisation, rate control, EXIF / ICC segments, entropy
 * coding on the device, encoding straight from the draw kernel.                                                           */

/* HOST functions (csrc/jpeg_host.cpp; no device access, safe to call from several threads at once).
 * rtm3d_jpeg_quality_tables: step 6 into q_luma[64] and q_chroma[64], natural order.
 * rtm3d_jpeg_frame_layout: the coefficient-buffer layout of an (h, w, mode) frame, as rtm3d_jpeg_info reports it for a stream
 * (restart_interval 0).
 * rtm3d_jpeg_encode_bound: the bound above for a stream with a restart interval of `restart` MCUs (0: none).
 * rtm3d_jpeg_entropy_encode: step 7 of the buffer h_coef (its tables included) into out[0 .. *bytes).  Refused with a reason:
 * an unknown mode, h or w outside 1..16384, restart outside 0..65535, a table entry of 0 or above 255, a DC difference of a
 * category above 11 or an AC coefficient of a category above 10 (|v| >= 1024; after a refusal of these two kinds the output
 * holds a partial stream), a capacity below rtm3d_jpeg_encode_bound.  Nothing outside out[0 .. capacity) is written and
 * nothing outside h_coef[0 .. coef_count) is read.                                                                        */
int rtm3d_jpeg_quality_tables(int quality, uint16_t* q_luma, uint16_t* q_chroma);
int rtm3d_jpeg_frame_layout(int h, int w, int mode, rtm3d_jpeg_stream_info* out);
int rtm3d_jpeg_encode_bound(int h, int w, int mode, int restart, size_t* bytes);
int rtm3d_jpeg_entropy_encode(const int16_t* h_coef, int h, int w, int mode, int restart, uint8_t* out, size_t capacity, size_t* bytes);

/* The device stage alone (csrc/jpeg_enc.hip): steps 1-5 for B frames.  h_frames[B] is a HOST array; d_src a DEVICE pointer to
 * h * w * 3 bytes at any address, d_coef a DEVICE pointer, 16-byte aligned, to the frame's coef_count int16.  q_luma[64] and
 * q_chroma[64] are HOST arrays, natural order.  Frames of different sizes and modes may share a chunk.  Stream-ordered, no
 * host synchronisation.
 * rtm3d_frames_jpeg_fdct_plan: the schedule of a batch, the very numbers the launcher uses; out[(B + 31) / 32] receives one
 * entry per chunk.  A frame is cut into tiles of tile_w x tile_h pixels - whole MCUs in every mode.  A workgroup of `threads`
 * converts its tile into Y and downsampled Cb / Cr planes in LDS (rows of lds_stride bytes; subsampled chroma lds_stride_sub),
 * every thread 8 pixels of 4 consecutive rows, and then runs the forward DCT and the quantisation of every block under the
 * tile, one block per thread and step.  Workgroup t of grid row i (frame first + i) takes tile t % tiles_x of tile row
 * t / tiles_x, tiles_x = ceil(w / tile_w), and leaves when t >= the frame's own number of tiles.  tiles is the largest of the
 * chunk, grid_x = tiles, grid_y = count.  (d_src, d_coef are not looked at.)
 * rtm3d_frames_jpeg_fdct_check: every refusal of rtm3d_frames_jpeg_fdct, without a launch: B < 1, a NULL array, source or
 * coefficient buffer, a buffer that is not 16-byte aligned, an unknown mode or src_order, reserved != 0, h or w outside
 * 1..16384, a table entry of 0 or above 255.  The message names the frame.                                                */
typedef struct rtm3d_jpeg_enc_frame {
    const uint8_t* d_src;                  /* DEVICE */
    int16_t* d_coef;                       /* DEVICE */
    int h, w, mode, reserved;              /* reserved = 0 */
} rtm3d_jpeg_enc_frame;
typedef struct rtm3d_jpeg_enc_plan {
    int first, count;                      /* frames first .. first + count - 1 */
    int tile_w, tile_h;                    /* 128 x 64 pixels */
    int threads;                           /* per workgroup */
    int lds_stride, lds_stride_sub;        /* 144, 72 */
    int tiles;                             /* tiles of the chunk's largest frame */
    int grid_x, grid_y;
} rtm3d_jpeg_enc_plan;
int rtm3d_frames_jpeg_fdct_plan(int B, const rtm3d_jpeg_enc_frame* h_frames, rtm3d_jpeg_enc_plan* out);
int rtm3d_frames_jpeg_fdct_check(int B, const rtm3d_jpeg_enc_frame* h_frames, const uint16_t* q_luma, const uint16_t* q_chroma, int src_order);
int rtm3d_frames_jpeg_fdct(void* stream, int B, const rtm3d_jpeg_enc_frame* h_frames, const uint16_t* q_luma, const uint16_t* q_chroma,
                           int src_order);

/* The chain: B packed frames h_src[b] on the device ((h, w) = h_hw[2 b], h_hw[2 b + 1]; one mode, one pair of tables, one
 * restart interval for the batch) to B streams in caller-owned HOST buffers h_out[b][0 .. h_out_capacity[b]), their lengths
 * in h_out_bytes[b].
 *   1. every refusal that needs no encoding, for the whole batch, before the first launch: those of the device stage, a
 *   capacity (bytes of d_coef and of h_stage) below rtm3d_jpeg_encode_workspace_bytes, an output below
 *   rtm3d_jpeg_encode_bound;  2. per chunk of 32 frames rtm3d_frames_jpeg_fdct into d_coef (frame b at the int16 offset that
 *   is the sum of the coef_count before it) and one hipMemcpyAsync of the chunk's buffers to the same offset of h_stage;
 *   3. an event behind the last copy, and the host waits on that event and on nothing else;  4. rtm3d_jpeg_entropy_encode of
 *   the B buffers on n_threads host threads (0: min(B, 8); at most 64).
 * The wait is inherent - the result is host bytes.  d_coef is a DEVICE buffer, 128-byte aligned; h_stage caller-owned HOST
 * memory of as many bytes - pinned, or the copies are not asynchronous.
 * The two halves are exported for pipelines that encode batch n while batch n + 1 runs: rtm3d_frames_jpeg_encode_queue is
 * steps 1 (without the outputs) and 2 and waits for nothing; rtm3d_frames_jpeg_encode_finish is step 4 alone, host only,
 * to be called once an event the CALLER recorded behind the queue call has completed.                                     */
int rtm3d_jpeg_encode_workspace_bytes(int B, const int* h_hw, int mode, size_t* bytes);
int rtm3d_frames_jpeg_encode(void* stream, int B, const uint8_t* const* h_src, const int* h_hw, int mode, const uint16_t* q_luma,
                             const uint16_t* q_chroma, int src_order, int restart, int16_t* d_coef, int16_t* h_stage, size_t capacity,
                             uint8_t* const* h_out, const size_t* h_out_capacity, size_t* h_out_bytes, int n_threads);
int rtm3d_frames_jpeg_encode_queue(void* stream, int B, const uint8_t* const* h_src, const int* h_hw, int mode, const uint16_t* q_luma,
                                   const uint16_t* q_chroma, int src_order, int16_t* d_coef, int16_t* h_stage, size_t capacity);
int rtm3d_frames_jpeg_encode_finish(int B, const int* h_hw, int mode, int restart, const int16_t* h_stage, uint8_t* const* h_out,
                                    const size_t* h_out_capacity, size_t* h_out_bytes, int n_threads);

/* ------------------------------------------------------------------ lens undistortion (csrc/lens.hip, csrc/engine.cpp)
 * Every other entry point takes a frame for a pinhole image described by a 3 x 3 K.  A frame of a real camera is one only
 * after rectification: this section builds rectifying maps on the device and resamples packed frames through them, the stage
 * between rtm3d_frames_convert and rtm3d_engine_detect_frames.  One launch per chunk of 32 frames, descriptors by value, no
 * host synchronisation.  Added in ABI 9 without changing any existing declaration, plan, engine file, record or default.
 *
 * THE MAP is plain data: ho * wo * 2 int32 on the device, 4-byte aligned.  Entry 2 * (y * wo + x) is sx, the next one sy:
 * the position in the SOURCE frame that destination pixel (x, y) is sampled from, in units of 1/32 pixel; integer
 * coordinates are pixel centres.  sx == RTM3D_LENS_OUTSIDE (INT32_MIN) means "no source"; any other int32 pair is legal.
 * A map may come from elsewhere (a table of another lens model, scaled by 32 and rounded): the remap asks nothing of it.
 *
 * THE REMAP RULE (integers only, int32, >> arithmetic; tests/lens_ref.py restates it in numpy).  Destination pixel (x, y),
 * channel c, of a source of h x w pixels:
 *   sx == INT32_MIN:  out = fill[c].  Otherwise
 *   ix = sx >> 5, ax = sx & 31, iy = sy >> 5, ay = sy & 31,
 *   S(i, j) = src[(j * w + i) * 3 + c] if 0 <= i < w and 0 <= j < h, else fill[c]   (decided per sample),
 *   out = ((32-ax)*(32-ay)*S(ix,iy) + ax*(32-ay)*S(ix+1,iy) + (32-ax)*ay*S(ix,iy+1) + ax*ay*S(ix+1,iy+1) + 512) >> 10.
 * The four weights sum to 1024, so out <= 255.  A sample of weight 0 need not be read; reads stay inside the h * w * 3 bytes of
 * each source; exactly ho * wo * 3 bytes are written per frame; sources and destinations may be any byte address.
 *
 * REFUSALS of the remap, checked for the whole batch before the first launch (the message names the frame; a refused call has
 * launched nothing): a NULL pointer (source, destination, map, fill), a side of the source or of the map < 1 or > 16384, a
 * map address that is no multiple of 4, reserved != 0, a destination that overlaps its own source.
 *
 * THE MAP BUILDER (fp64, one fixed operation order, compiled without contraction; + - * / are IEEE, so the two polynomial
 * models are defined bit for bit; sqrt and atan of the fisheye model are the device library's).  R (row-major) takes a ray
 * of the RECTIFIED camera to a ray of the PHYSICAL camera - the transpose of the matrix OpenCV's initUndistortRectifyMap
 * is given; the identity when there is no rectifying rotation.  Kr = the rectified camera's K.  Destination pixel (u, v),
 * every line evaluated left to right as written:
 *   a = ((double)u - Kr[2]) / Kr[0],  b = ((double)v - Kr[5]) / Kr[4]
 *   X = R[0]*a + R[1]*b + R[2],  Y = R[3]*a + R[4]*b + R[5],  Wz = R[6]*a + R[7]*b + R[8]
 *   !(Wz > 0): OUTSIDE.   x = X / Wz,  y = Y / Wz
 * RTM3D_LENS_BROWN, dist = k1 k2 p1 p2 k3 k4 k5 k6 (the rational model; zeros give the 5-parameter one):
 *   r2 = x*x + y*y,  num = 1 + r2*(k1 + r2*(k2 + r2*k3)),  den = 1 + r2*(k4 + r2*(k5 + r2*k6)),  cdist = num / den
 *   xd = x*cdist + ((2*p1)*x*y + p2*(r2 + (2*x)*x)),  yd = y*cdist + (p1*(r2 + (2*y)*y) + (2*p2)*x*y)
 * RTM3D_LENS_FISHEYE (Kannala-Brandt equidistant), dist = k1 k2 k3 k4 0 0 0 0:
 *   r = sqrt(x*x + y*y),  t = atan(r),  t2 = t*t,  td = t*(1 + t2*(k1 + t2*(k2 + t2*(k3 + t2*k4))))
 *   s = r > 1e-8 ? td / r : 1,  xd = x*s,  yd = y*s
 * Both:  U = K[0]*xd + K[2],  V = K[4]*yd + K[5];  either not finite or above 2^20 in magnitude: OUTSIDE; otherwise
 *   sx = (int32)floor(U*32.0 + 0.5),  sy = (int32)floor(V*32.0 + 0.5).
 * An OUTSIDE entry is written as the pair (INT32_MIN, INT32_MIN).
 * REFUSALS of the builder, before the first launch (the message names the map): an unknown kind; in K or Kr an entry [1], [3],
 * [6] or [7] that is not 0, [8] that is not 1, fx or fy that is not > 0; a side of the lens or of the map < 1 or > 16384; a
 * non-zero entry among the last four of a fisheye dist; a NULL or misaligned map.
 *
 * OUT OF SCOPE: choosing an "optimal" new camera matrix (callers pass Kr); filters other than this bilinear; fusing the remap
 * into the pixel-format conversion; taking records back into the raw, distorted frame; parity with OpenCV's remap and
 * initUndistortRectifyMap - the rules above restate the textbook models, OpenCV was not at hand to pin them against (as
 * with the KITTI and TrackEval restatements): the fixed-point weights (5 bits here) and the rounding differ by design.    */
#define RTM3D_LENS_OUTSIDE INT32_MIN
#define RTM3D_LENS_BROWN 0
#define RTM3D_LENS_FISHEYE 1
typedef struct rtm3d_lens_map {
    const int32_t* d_map;                  /* DEVICE pointer: ho * wo pairs (sx, sy) */
    int ho, wo;                            /* the size of the frame the map makes */
    int reserved;                          /* 0 */
} rtm3d_lens_map;
typedef struct rtm3d_lens_model {          /* the physical camera */
    int kind;                              /* RTM3D_LENS_BROWN | RTM3D_LENS_FISHEYE */
    int h, w;                              /* the size of its frames */
    double K[9];                           /* row-major 3 x 3, no skew */
    double dist[8];
} rtm3d_lens_model;
typedef struct rtm3d_lens_rect {           /* the pinhole image made */
    int ho, wo;
    double K[9];                           /* Kr */
    double R[9];                           /* rectified ray -> physical ray */
} rtm3d_lens_rect;

/* rtm3d_frames_remap_plan: the schedule rtm3d_frames_remap gives a batch - the very numbers the launcher uses, it calls the
 * same code; out[(B + 31) / 32] receives one entry per chunk.  A destination row is cut into runs of px_per_thread
 * consecutive pixels; thread t = block * threads + lane of grid row i (frame first + i) takes run t % runs_per_row of row
 * t / runs_per_row, runs_per_row = ceil(wo / px_per_thread), and leaves when t >= the frame's own number of runs.  runs is
 * the largest of the chunk, grid_x = ceil(runs / threads), grid_y = count.  The maps are validated as by rtm3d_frames_remap.
 * rtm3d_frames_remap_check: every refusal of rtm3d_frames_remap, without a launch.                                      */
typedef struct rtm3d_remap_plan {
    int first, count;                      /* frames first .. first + count - 1 */
    int px_per_thread;                     /* 4 consecutive pixels of one row: 32 B of map, 12 B of output */
    int threads;                           /* per workgroup */
    int runs;                              /* thread runs of the chunk's largest destination */
    int grid_x, grid_y;
} rtm3d_remap_plan;
int rtm3d_frames_remap_plan(int B, const rtm3d_lens_map* h_maps, rtm3d_remap_plan* out);
int rtm3d_frames_remap_check(int B, const uint8_t* const* h_src, const int* h_hw, const rtm3d_lens_map* h_maps,
                             uint8_t* const* h_dst, const uint8_t fill[3]);

/* The remap: h_src[B] HOST array of DEVICE pointers to packed uint8 (h, w, 3) frames (the output of rtm3d_frames_convert, for
 * one), h_hw[2B] their (h, w), h_maps[B] (frames may share a map), h_dst[b] a DEVICE pointer to ho * wo * 3 packed bytes.
 * Stream-ordered.                                                                                                       */
int rtm3d_frames_remap(void* stream, int B, const uint8_t* const* h_src, const int* h_hw, const rtm3d_lens_map* h_maps,
                       uint8_t* const* h_dst, const uint8_t fill[3]);

/* The builder: map i of n, h_maps[i] a DEVICE pointer to ho * wo * 2 int32, from lens h_models[i] and rectified camera
 * h_rect[i] (all HOST arrays).  One launch per chunk of 8 maps, descriptors by value, stream-ordered.                   */
int rtm3d_lens_map_build(void* stream, int n, const rtm3d_lens_model* h_models, const rtm3d_lens_rect* h_rect,
                         int32_t* const* h_maps);

/* One detect step of an engine fed by frames of a real lens: with h_src != NULL rtm3d_frames_convert into h_packed[B] (h_hw is
 * ignored, the sizes are the sources'); with h_src == NULL h_packed[B] already holds the raw packed frames of sizes h_hw[2B].
 * Then rtm3d_frames_remap of h_packed through h_maps[B] into h_rect[B] (DEVICE buffers of ho * wo * 3 bytes), then
 * rtm3d_engine_detect_frames on h_rect with the maps' (ho, wo) and d_K_rect (B x 9 fp64, the RECTIFIED cameras' intrinsics).
 * Records and KITTI rows are in the pixels and the camera of the rectified frames - the frames the drawing entry points
 * then paint into.  Same workspace, same rtm3d_engine_set_frame_params, no host synchronisation; everything the three steps
 * would refuse is refused before the first launch.                                                                      */
int rtm3d_engine_detect_frames_lens(rtm3d_ctx* ctx, void* stream, const rtm3d_frame_src* h_src, uint8_t* const* h_packed,
                                    const int* h_hw, int dst_order, const rtm3d_lens_map* h_maps, uint8_t* const* h_rect,
                                    const uint8_t fill[3], const double* d_K_rect, float* d_rec, double* d_kitti,
                                    void* d_workspace);

/* ------------------------------------------------------------------ box overlaps (csrc/box_overlap.hip)
 * Rotated-box overlaps in the ground plane and 3D non-maximum suppression of detection records.  Added in ABI 9 without
 * changing any existing declaration; nothing calls these unless the caller does (no plan, engine file or record changes).
 *
 * BOX: 7 values in the order of record fields [24:31] - h, w, l, X, Y, Z, ry.  (X, Y, Z) is the box CENTRE in camera
 * coordinates (y down), as rtm3d_pack_records writes it (a KITTI label line carries the bottom face instead: y + h / 2).
 * The footprint lies in the x-z plane: half extents l / 2 along local x and w / 2 along local z, rotated by
 * R = [[c,0,s],[0,1,0],[-s,0,c]] with plain c = cos(ry), s = sin(ry) - NOT the rotation_matrix of the reference's drawing
 * code, which snaps |s|, |c| < 1e-3 to zero.  Vertical extent [Y - h / 2, Y + h / 2].
 * ARITHMETIC: fp64 throughout, one fixed operation order for both entry points, compiled without contraction.  The BEV
 * intersection is rectangle A clipped against the four half-planes of B (Sutherland-Hodgman, at most 8 vertices) with CLOSED
 * inside tests (>= 0): identical boxes, boxes sharing an edge and nested boxes give the exact intersection, not an empty
 * polygon.  3D intersection = BEV intersection * overlap of the vertical extents.  A box with h, w or l <= 0 or with any
 * non-finite value overlaps nothing (0); a denominator of 0 gives 0; no result is NaN.
 *
 * rtm3d_box_overlaps: per image two ragged lists d_a [B][cap_a][7], d_b [B][cap_b][7] with d_na[B], d_nb[B] valid entries.
 * criterion: 0 = intersection / union, 1 = intersection / size of a, 2 = intersection / size of b (KITTI's -1 / 0 / 1 cases);
 * "size" is the footprint area for d_bev and the volume for d_3d.  Outputs [B][cap_a][cap_b] fp64, either may be NULL (not
 * both); entries with i >= d_na[image] or j >= d_nb[image] are written as 0, so the outputs are fully defined.  One lane per
 * pair, one launch.  (These matrices feed the BEV / 3D scores of the KITTI evaluation: rtm3d_kitti_match below does the matching
 * on them, rtm3d_amd/kitti_eval.py the difficulty filtering and the AP integral.)
 *
 * rtm3d_records_nms3d: greedy NMS in place on B * topk * 32 records (rtm3d_pack_records, before or after
 * rtm3d_records_to_camera, local or all-gathered: B is just the number of images).  Candidates are the slots with flag
 * [31] == 2; their boxes are fields [24:31] widened to fp64 (exact), so the arithmetic is that of rtm3d_box_overlaps on
 * (double)rec[24:31].  Slots are score-descending within an image (rtm3d_decode2d; ties by flat index): slot i survives if
 * no SURVIVING slot j < i has IoU STRICTLY GREATER than iou_thresh with it.  metric: 0 = BEV IoU, 1 = 3D IoU.
 * class_aware != 0: only boxes of the same class [0] suppress each other.  A suppressed slot's flag goes 2 -> 1 and nothing
 * else of the record changes, so it still reads as "a detection" (> 0) and no longer as "3D kept" (> 1).  NOTE: a flag-1
 * slot may therefore carry a 3D box in [24:31] that is not kept - as it already may after rtm3d_pack_records, which writes
 * the solver's output of a solved-but-rejected slot (fun >= fun_accept) into those fields.  d_kitti (NULL or the B * topk *
 * 16 rows of rtm3d_records_to_camera): the row of a suppressed slot is zeroed, that array's rule for not-kept slots - the
 * same rows rtm3d_records_to_camera writes when it runs after this entry, since it gives a row to flag-2 slots only.
 * One workgroup per image; topk > 256 is refused.  Stream-ordered: one kernel, no host synchronisation, no memset / memcpy
 * node, no allocation.                                                                                                      */
int rtm3d_box_overlaps(void* stream, int B, int cap_a, int cap_b, const int32_t* d_na, const int32_t* d_nb,
                       const double* d_a, const double* d_b, int criterion, double* d_bev, double* d_3d);
int rtm3d_records_nms3d(void* stream, int B, int topk, float* d_rec, double iou_thresh, int metric, int class_aware,
                        double* d_kitti);

/* ------------------------------------------------------------------ KITTI evaluation (csrc/kitti_eval.hip)
 * The device side of the KITTI object-detection AP protocol (bbox / BEV / 3D / AOS); the host side - label files, difficulty
 * filtering, score thresholds, the AP integral - is rtm3d_amd/kitti_eval.py.  Added in ABI 9 without changing any existing
 * declaration; nothing calls these unless the caller does.  The protocol is restated from the published devkit's behaviour;
 * that program was not available to compare against, so parity with it is UNPINNED: the contract is the rules written here.
 * Both entry points are stream-ordered: one kernel, no host synchronisation, no memset / memcpy node, no allocation.
 *
 * rtm3d_rect_overlaps: pairwise overlaps of axis-aligned image rectangles (x1, y1, x2, y2), layout as rtm3d_box_overlaps:
 * d_a [B][cap_a][4], d_b [B][cap_b][4], d_na[B], d_nb[B] valid entries, d_out [B][cap_a][cap_b] fp64; entries with
 * i >= d_na[image] or j >= d_nb[image] are written as 0.  fp64 in this order, compiled without contraction:
 *   w = fmin(ax2, bx2) - fmax(ax1, bx1);  h = fmin(ay2, by2) - fmax(ay1, by1);  w <= 0 or h <= 0 -> 0;
 *   inter = w * h;  sa = (ax2 - ax1) * (ay2 - ay1);  sb = (bx2 - bx1) * (by2 - by1);
 *   criterion 0: inter / ((sa + sb) - inter)   1: inter / sa   2: inter / sb.
 * A rectangle with a coordinate that is not finite overlaps nothing (0); a denominator that is zero or not finite gives 0,
 * and so does a quotient that is not finite: no result is NaN or infinite.  There is no "+1" pixel convention.
 *
 * rtm3d_kitti_match: the greedy matching.  It computes no overlap itself: d_overlap [n_frames][cap_d][cap_g] fp64 is one
 * matrix per frame (detection x ground truth) of whatever metric.  One ITEM is one (frame, group): item = frame * n_groups +
 * group, a group being one (class, difficulty).  cap_d <= 256, more is refused; cap_g is not limited.
 *   d_nd / d_ng [n_frames]           detections / ground truths of the frame (entries beyond them are never read)
 *   d_gflag [n_frames][n_groups][cap_g], d_dflag [n_frames][n_groups][cap_d]   int8: 0 counted, 1 ignored, -1 other class
 *   d_score [n_frames][cap_d]        fp64 detection scores; they must be finite
 *   d_dc_hit [n_frames][n_groups][cap_d] or NULL   uint8, 1: the detection overlaps a DontCare region beyond min_overlap
 *   d_alpha_g [n_frames][cap_g], d_alpha_d [n_frames][cap_d], both or neither   observation angles (AOS only)
 *   d_min_overlap [n_groups]         fp64, >= 0
 * The ground truths of an item are walked in index order; one with flag -1 is skipped.  ELIGIBLE for a ground truth g: the
 * detections that are not assigned yet, have flag != -1 and overlap[d][g] > min_overlap (strict).
 * mode 0, SCORES (the devkit's compute_fp = false), one wavefront per item.  Candidate: the eligible detection of highest
 * score; strict >, so the lowest index wins a tie.  No candidate: a miss.  A candidate and (gflag == 1 or its dflag == 1): the
 * detection becomes assigned, nothing is counted.  Otherwise a true positive: the detection becomes assigned and its score
 * is written to d_match_score[item][g].  Every other entry of d_match_score [n_frames][n_groups][cap_g] is -infinity.
 * max_thr and the counts-mode pointers are not used.
 * mode 1, COUNTS (compute_fp = true), one wavefront per (item, k), k < d_nthr[group] <= max_thr, with the threshold
 * t = d_thr[group][k] of d_thr [n_groups][max_thr]: detections with score < t (strict) do not exist.  Candidate: if any
 * eligible detection has flag 0, the one of largest overlap among those (strict >: lowest index at a tie); otherwise the
 * lowest-index eligible detection with flag 1 - the closed form of the devkit's sequential max_overlap /
 * assigned_ignored_det update.  Miss / assign-only / true positive as in scores mode; a true positive adds
 * (1 + cos(alpha_g - alpha_d)) / 2 to the item's similarity (0 without the angles).  After the walk, the false positives are
 * the detections with flag 0, score >= t, not assigned and not d_dc_hit.
 * Outputs: d_tp / d_fp / d_fn [n_groups][max_thr] int32 are ADDED TO (vector atomics; the caller zeroes them, and may run
 * several frame chunks into the same arrays); d_sim [n_frames][n_groups][max_thr] fp64 holds the similarity of every
 * (item, k), 0 for k >= d_nthr[group], for the caller to sum.  d_match_score is not used.                                 */
int rtm3d_rect_overlaps(void* stream, int B, int cap_a, int cap_b, const int32_t* d_na, const int32_t* d_nb,
                        const double* d_a, const double* d_b, int criterion, double* d_out);
int rtm3d_kitti_match(void* stream, int mode, int n_frames, int n_groups, int cap_d, int cap_g, const int32_t* d_nd,
                      const int32_t* d_ng, const int8_t* d_gflag, const int8_t* d_dflag, const double* d_score,
                      const uint8_t* d_dc_hit, const double* d_alpha_g, const double* d_alpha_d, const double* d_overlap,
                      const double* d_min_overlap, double* d_match_score, int max_thr, const int32_t* d_nthr,
                      const double* d_thr, int32_t* d_tp, int32_t* d_fp, int32_t* d_fn, double* d_sim);

/* ------------------------------------------------------------------ drawing (csrc/draw.hip)
 * Detection records painted into the camera frames and into a bird's-eye panel, on the device: the counterpart of the
 * reference's utils/visual_utils.py (key points, 2D boxes, the eight vertices as a wireframe with a shaded front face, the
 * solved box through the camera, a bird's-eye view).  Added in ABI 9 without changing any existing declaration; nothing calls
 * this unless the caller does (no plan, engine file or record changes).  The rule below is the project's own and replaces
 * OpenCV's rasteriser, whose pixel values were never pinned here: everything is an integer, so the result is defined BIT FOR
 * BIT.  OUT OF SCOPE: text labels (there is no font in the library), anti-aliasing, clipping of boxes that cross the image
 * plane, the reference's heat-map overlays.  (Text labels and track colours: rtm3d_records_draw_tracks, "drawing tracks" below.)
 *
 * FRAMES: h_imgs[B] HOST array of DEVICE pointers to uint8 (h, w, 3) frames, contiguous, h_hw[2B] their (h, w), as for
 * rtm3d_engine_detect_frames; painted IN PLACE.  The channel order is the caller's and colours are given in the same order.
 * A side longer than 8192 (or < 1) is refused with an error that names the frame; the whole batch is checked first.
 * d_rec: B * topk * 32 records in the pixels of each frame (the output of rtm3d_engine_detect_frames).
 * PAINTER'S ORDER: the result is that of painting the slots of an image one after the other FROM THE LAST TO THE FIRST - slot
 * 0, the best score, ends on top - and within a slot the layers in the order front-face shade, 2D box, wireframe, key-point
 * disc.  Only slots with flag [31] >= min_flag are painted (1 = every detection, 2 = 3D-kept only).  Empty slots and images
 * without a detection leave the frame untouched, byte for byte.
 * COORDINATES: a coordinate becomes an integer by truncation toward zero (the reference's astype(int)).  A primitive - one
 * segment, one disc, one face - with a coordinate that is not finite or whose integer lies outside [-8192, 8192] is not
 * drawn; the other primitives of the slot are.
 * COLOUR: color[class] with class = (int)[0]; ncls = the number of RGB triples in the table (1..RTM3D_ENGINE_MAX_CLASSES,
 * anything else is refused).  The records are device memory and the call does not synchronise, so a RECORD whose class lies
 * outside [0, ncls) cannot be turned into a return code: such a slot is not drawn (rtm3d_amd.draw.draw_records checks the
 * classes on the host and raises).
 * LAYERS (bit mask `layers`):
 *   thick segment P-Q of thickness t: covers pixel p iff the squared distance from p to the closed segment is <= t^2 / 4,
 *     in integers: d = Q - P, v = p - P, k = v.d;  k <= 0: 4 |v|^2 <= t^2;  k >= d.d: 4 |p - Q|^2 <= t^2;  otherwise
 *     (2 (v x d))^2 <= t^2 (d.d).  P == Q is the disc of radius t / 2 (first case).  With t = 1 the cover is gap-free: along
 *     the major direction some pixel centre lies within 0.5 of the line in every column (row).  (Ranges: csrc/draw.hip.)
 *   RTM3D_DRAW_KEYPOINT  disc |p - c|^2 <= radius^2 at [2:4] (radius 0..64);
 *   RTM3D_DRAW_BOX2D     the four sides of [20:24] = (x1, y1, x2, y2) as thick segments of `thickness` (1..15);
 *   RTM3D_DRAW_WIREFRAME the twelve edges 01 13 32 20 04 45 57 76 64 51 37 62 of the box over vertices 0..7 - the edges the
 *     reference's outline path 0 1 3 2 0 4 5 7 6 4 5 1 3 7 6 2 traces, each once - as thick segments of `thickness`;
 *   RTM3D_DRAW_FACE      the front face, vertices 0 1 3 2: a pixel is covered iff it lies in the closed triangle (0, 1, 3) or
 *     in the closed triangle (0, 3, 2) - integer edge functions (b - a) x (p - a), all three >= 0 or all three <= 0; a
 *     triangle of zero area covers nothing - and becomes (px * (256 - a) + colour * a + 128) >> 8 per channel, a =
 *     face_alpha (0..256), ONCE per slot.  Slots are painted in sequence, so overlapping faces compound by this formula.
 *   The vertices: source 0 = the regressed vertices [4:20]; source 1 = the solved box [24:31] widened to fp64 and projected
 *     through d_K_camera (B x 9 fp64; may be NULL unless source == 1) with the corner order and operation sequence of
 *     rtm3d_project_boxes (csrc/box_project.h) on x = [., ., l, h, w, X, Y, Z], fed with PLAIN sin(ry) and cos(ry) (no snap
 *     of small values), compiled without contraction.  Source 1 draws wireframe and face for slots with flag 2 only, and a
 *     slot with any corner at camera depth Z below 0.1 (or NaN) gets neither: there is no clipping against the image plane.
 *   RTM3D_DRAW_BEV       the bird's-eye panel: d_bev (may be NULL unless this bit is set), B caller-owned uint8 (bev_h, bev_w,
 *     3) images (sides 1..8192), painted in place by the same rules, slots with flag 2 (and >= min_flag) only.  The footprint
 *     is that of "box overlaps": half extents hl = l / 2 along local x, hw = w / 2 along local z, c = cos(ry), s = sin(ry);
 *     a local point (lx, lz) lies at world x = (c * lx + s * lz) + X, z = (c * lz - s * lx) + Z.  The corners (hl, hw),
 *     (-hl, hw), (-hl, -hw), (hl, -hw), the centre (X, Z) and the midpoint (hl, 0) of the +x edge are mapped by
 *     u = trunc(bev_w / 2. + x / m), v = trunc(bev_h - z / m), m = bev_m_per_px (fp64, positive): the outline is the four
 *     segments between consecutive corners, the heading mark the segment centre - midpoint, all of thickness 1.
 * rtm3d_draw_default_params: the four frame layers, source 0, min_flag 1, thickness 1, radius 5, face_alpha 77, a palette of
 * the project's own choosing for all RTM3D_ENGINE_MAX_CLASSES classes, no panel.
 * rtm3d_records_draw: one launch per 64 frames, one workgroup per 64 x 16 tile of a frame or panel that gathers the
 * primitives touching it (a tile none touches neither reads nor writes memory).  Stream-ordered: no host synchronisation, no
 * memset / memcpy node, no allocation.  Bad arguments return non-zero with the reason in rtm3d_last_error().              */
#define RTM3D_DRAW_FACE 1
#define RTM3D_DRAW_BOX2D 2
#define RTM3D_DRAW_WIREFRAME 4
#define RTM3D_DRAW_KEYPOINT 8
#define RTM3D_DRAW_BEV 16
typedef struct rtm3d_draw_params {
    int layers, source, min_flag, thickness, radius, face_alpha, ncls;
    uint8_t color[RTM3D_ENGINE_MAX_CLASSES][3];
    int bev_h, bev_w;
    double bev_m_per_px;
} rtm3d_draw_params;
int rtm3d_draw_default_params(rtm3d_draw_params* p);
int rtm3d_records_draw(void* stream, int B, int topk, const float* d_rec, uint8_t* const* h_imgs, const int* h_hw,
                       const double* d_K_camera, const rtm3d_draw_params* params, uint8_t* d_bev);

/* ------------------------------------------------------------------ tracking (csrc/track.hip)
 * The kept 3D boxes of the records followed from frame to frame on the device: an identity and a velocity per object, by the
 * tracking-by-detection baseline of the KITTI 3D trackers (a constant-velocity Kalman filter per object, a greedy match of this
 * frame's boxes to the live tracks on 3D overlap or centre distance).  Added in ABI 9 without changing any existing
 * declaration; nothing calls these unless the caller does (no plan, engine file or record changes).  The records are READ ONLY.
 * The rule below is complete: tests/track_ref.py is written from it.  Everything is fp64, in the operation order written here,
 * compiled without contraction; "a * b + c" below means the rounded product, then the rounded sum, and sums associate left
 * to right unless bracketed.
 *
 * STREAMS: B independent streams, stream b = batch index b of the records.  d_state is caller-owned device memory,
 * rtm3d_tracks_state_bytes(B, T) bytes: per stream RTM3D_TRACK_HEADER_DOUBLES + T * RTM3D_TRACK_SLOT_DOUBLES doubles, T track
 * slots, 1 <= T <= 256.  An all-zero table is an empty stream: hipMemsetAsync of a stream's part is its reset.  LAYOUT, all fp64:
 *   header [0] ids issued so far (the next id is this + 1)  [1] frames seen  [2] dropped births so far  [3:8] zero
 *   slot   [0] id (0 = free slot, and then all 24 values are zero)  [1] class  [2] age in frames, 1 at birth  [3] hits = matched
 *          frames in a row, the birth included  [4] misses in a row  [5] score of the last matched detection  [6] record slot it
 *          matched in THIS frame, -1 if none  [7:10] h w l  [10:13] X Y Z  [13] ry  [14:17] vx vy vz (per unit of dt)
 *          [17] Ppp [18] Ppv [19] Pvv: the 2 x 2 (position, velocity) covariance all three axes share - what a filter started
 *          from isotropic diagonal noise stays equal to  [20] variance of ry  [21] variance shared by h, w, l  [22:24] zero
 * DETECTIONS of a frame: the record slots k < topk with flag [31] == 2 and (double)[1] >= min_score, in slot order; box
 * z = (double)[24:31] = h w l X Y Z ry (centre convention of "box overlaps"), class (double)[0].  The caller's boxes are taken
 * as they are: a box that is not finite makes a track that is not finite, matches nothing and dies of its misses.
 * wrap(a) = a - TWO_PI * floor((a + PI) / TWO_PI), PI = 3.141592653589793, TWO_PI = 6.283185307179586: [-pi, pi).
 *
 * One call = one frame of every stream, in these steps.  frame = header[1] + 1.
 * 1 PREDICT every live slot (id != 0), dt > 0 the time since the previous call:
 *     X = X + dt * vx (Y, Z alike);  age = age + 1;
 *     ego motion, if d_ego != NULL: e = d_ego + 12 * b is the row-major 3 x 4 [R | t] that takes a point of the previous
 *     frame's camera coordinates to the current frame's.  With the stepped position (x, y, z) and the velocity:
 *       X = ((e[0] * x + e[1] * y) + e[2] * z) + e[3]   (rows 1, 2 alike with e[4..7], e[8..11]);
 *       vx = (e[0] * vx + e[1] * vy) + e[2] * vz        (rows alike; all three from the old velocity);
 *       the heading vector (c, 0, -s), c = cos(ry), s = sin(ry), turns with R:  ry = atan2(-(e[8] * c - e[10] * s), e[0] * c - e[2] * s).
 *     The covariances are isotropic, so a rotation leaves them as they are.
 *     ry = wrap(ry)
 *     a = Ppp + dt * Ppv;  b = Ppv + dt * Pvv;  Ppp = (a + dt * b) + q_pos * dt;  Ppv = b;  Pvv = Pvv + q_vel * dt   (b, Pvv: old)
 *     Pry = Pry + q_ry * dt;  Pdim = Pdim + q_dim * dt.   h, w, l, class, id are kept.
 * 2 AFFINITY of every (live slot t, detection k), track first: metric 0 = BEV IoU, 1 = 3D IoU of the predicted box (h, w, l,
 *     X, Y, Z, ry of step 1) as box a and the detection as box b, by the arithmetic of rtm3d_box_overlaps, criterion 0 - with
 *     one shortcut: with (ex, ey, ez) = predicted centre - detection centre and
 *     reach = 0.5 * sqrt(w_a * w_a + l_a * l_a) + 0.5 * sqrt(w_b * w_b + l_b * l_b), a pair with ex * ex + ez * ez > reach * reach
 *     has affinity 0 (the footprints cannot meet; nothing is clipped).  metric 2 = -sqrt((ex * ex + ey * ey) + ez * ez), minus
 *     the centre distance.  The pair is a CANDIDATE iff affinity > thresh (strict; never for NaN) and, with class_aware != 0,
 *     slot class == detection class.
 * 3 MATCH: the sequential global greedy one - take the remaining candidate of highest affinity, the lower track slot at a tie,
 *     then the lower record slot; remove its track and its detection; repeat until no candidate remains.  (The kernel runs
 *     rounds of mutual best, which gives this result: csrc/track.hip.)
 * 3b MATCH, optimal (rtm3d_tracks_update_assign with RTM3D_TRACK_ASSIGN_OPTIMAL; steps 1, 2, 4, 5, 6 as they are, and the
 *     candidates exactly those of step 2).  The GAIN of a candidate pair is g(t, k) = affinity - thresh, strictly positive by
 *     the definition of a candidate.  A matching is a set of candidate pairs in which no track slot and no record slot appears
 *     twice; the match is a matching of the largest sum of gains, the sum associated as the implementation likes.  Leaving a
 *     track or a detection unmatched costs nothing, and a pair that is no candidate is never matched, so nothing is filtered
 *     afterwards.  This is NOT "solve the assignment on the full affinity matrix, then drop the pairs under the threshold":
 *     that rule spends tracks and detections on pairs it then throws away, while here a pair at or below the threshold is
 *     simply absent and its track and its detection stay free for others.  (Tracks A, B, detections x, y, centre distances
 *     A-x 1.0, B-x 1.2, A-y 2.1, B-y 3.0, thresh -2: the full matrix is solved by A-y and B-x, 3.3 against 4.0; A-y is dropped
 *     and B-x stays, gain 0.8.  The rule here has the candidates A-x and B-x only and matches A-x, gain 1.0.)
 *     Where several matchings attain the maximum, within the fp64 rounding of the sums, any one of them may be returned - the
 *     same one on every call with the same inputs: no result depends on the order in which lanes or atomics retire.  (The
 *     kernel runs shortest augmenting paths over the live slots that have a candidate, in slot order, taking the lowest record
 *     slot at equal slack: the solver of csrc/assign_wave.h.)  thresh must be finite under this rule (the gains are differences
 *     from it).
 * 4 UPDATE a matched slot with its detection z (zry = wrap(z ry)), everything on the right of one line from before that line:
 *     S = Ppp + r_pos;  Kp = Ppp / S;  Kv = Ppv / S
 *     per axis: y = zX - X;  X = X + Kp * y;  vx = vx + Kv * y
 *     Ppp' = Ppp - Kp * Ppp;  Ppv' = Ppv - Kp * Ppv;  Pvv' = Pvv - Kv * Ppv   (all three from the predicted values)
 *     heading: if |wrap(zry - ry)| > 1.5707963267948966: ry = wrap(ry + PI) - a box seen from the other end is the same box;
 *     y = wrap(zry - ry);  K = Pry / (Pry + r_ry);  ry = wrap(ry + K * y);  Pry = Pry - K * Pry
 *     K = Pdim / (Pdim + r_dim);  h = h + K * (zh - h) (w, l alike);  Pdim = Pdim - K * Pdim
 *     hits = hits + 1;  misses = 0;  [5] = detection score;  [6] = k.
 *   An UNMATCHED live slot keeps its predicted state: hits = 0, misses = misses + 1, [6] = -1; once misses > max_misses the slot
 *   is freed (all zero) - so a track survives max_misses frames without a detection and loses its id on the next.
 * 5 BIRTHS: the unmatched detections, in slot order, open tracks in the free slots, in slot order (slots freed in step 4 of
 *   this call included); the n-th of them (n = 1 ..) gets id = header[0] + n.  Ids start at 1 and are never reused.  A new
 *   slot: class, box and score of the detection, ry = wrap(z ry), velocity 0, Ppp = p0_pos, Ppv = 0, Pvv = p0_vel, Pry =
 *   p0_ry, Pdim = p0_dim, age 1, hits 1, misses 0, [6] = k.  When the free slots run out the remaining births are dropped -
 *   the lower scores, records being score-ordered - and counted: header[2] += dropped;  header[0] += births;  header[1] = frame.
 * 6 IDS: d_ids [B][topk] int32, one per record slot: 0 = not tracked (no detection, or a dropped birth); otherwise the id of the
 *   slot the detection was matched to or born into, +id if that track is CONFIRMED - hits >= min_hits, or frame <= min_hits -
 *   and -id while it is tentative.
 *
 * rtm3d_track_default_params: metric 1, thresh 0.01, class_aware 0, max_misses 2, min_hits 3, min_score 0, initial variances
 * position 10, velocity 1e4, ry 10, dimensions 10, process noise (per unit of dt) 0.01 on the velocity and 0 elsewhere,
 * measurement noise 1 - the usual baseline's.
 * rtm3d_tracks_update: two launches - the affinity matrix of all streams, one lane per (slot, record slot) pair, into d_ws
 * (rtm3d_tracks_workspace_bytes(B, topk, T) bytes, fully rewritten by every call); then one workgroup per stream for steps 1
 * and 3 - 6.  Stream-ordered: no host synchronisation, no memset / memcpy node, no allocation.  topk <= 256 and T <= 256, more is
 * refused.  Refused before anything is launched, non-zero with the reason in rtm3d_last_error(): B < 1, T or topk outside
 * 1..256, dt not positive and finite, a NULL d_rec / params / d_state / d_ids / d_ws, metric outside 0..2, negative max_misses
 * or min_hits, NaN thresh or min_score, a variance or process noise that is negative or not finite, measurement noise that is
 * not positive and finite.  The two size functions return 0 for sizes the update would refuse.
 * rtm3d_tracks_update_assign (additive, still ABI 9): the same call with the rule of step 3 chosen by `assign`.
 * RTM3D_TRACK_ASSIGN_GREEDY is rtm3d_tracks_update itself - the same two kernels, the same results bit for bit;
 * RTM3D_TRACK_ASSIGN_OPTIMAL runs step 3b in place of step 3, in the same two launches, the same workspace and without a host
 * synchronisation.  Every refusal of rtm3d_tracks_update applies, in its words; refused too, before anything is launched: an
 * assign outside 0..1 (the value is in rtm3d_last_error()) and, under the optimal rule, a thresh that is not finite.        */
#define RTM3D_TRACK_HEADER_DOUBLES 8
#define RTM3D_TRACK_SLOT_DOUBLES 24
typedef struct rtm3d_track_params {
    int metric, class_aware, max_misses, min_hits;
    double thresh, min_score;
    double p0_pos, p0_vel, p0_ry, p0_dim;
    double q_pos, q_vel, q_ry, q_dim;
    double r_pos, r_ry, r_dim;
} rtm3d_track_params;
int rtm3d_track_default_params(rtm3d_track_params* p);
size_t rtm3d_tracks_state_bytes(int B, int T);
size_t rtm3d_tracks_workspace_bytes(int B, int topk, int T);
int rtm3d_tracks_update(void* stream, int B, int topk, int T, const float* d_rec, double dt, const double* d_ego /* or NULL */,
                        const rtm3d_track_params* params, double* d_state, int32_t* d_ids, void* d_ws);
#define RTM3D_TRACK_ASSIGN_GREEDY 0
#define RTM3D_TRACK_ASSIGN_OPTIMAL 1
int rtm3d_tracks_update_assign(void* stream, int B, int topk, int T, const float* d_rec, double dt, const double* d_ego /* or NULL */,
                               const rtm3d_track_params* params, int assign, double* d_state, int32_t* d_ids, void* d_ws);

/* ------------------------------------------------------------------ drawing tracks (csrc/draw_tracks.hip)
 * rtm3d_records_draw with what a tracker adds: a stable colour per track id, a text label per slot, and a bird's-eye panel painted
 * from the track table - coasting tracks, the filtered box, the velocity.  Additive (still ABI 9): rtm3d_records_draw and its
 * parameters are as they were, and nothing calls this unless the caller does.  Everything of "drawing" holds - frames, records,
 * coordinates (COORD below = its rule: truncation toward zero; a value that is not finite or whose integer lies outside [-8192,
 * 8192] is BAD), the thick segment, the layers, the panel mapping - and the rule below is complete with it: tests/draw_tracks_ref.py
 * is written from the two sections.  All results are integers, defined bit for bit.
 *
 * d_ids [B][topk] int32: the ids of "tracking", step 6, for the same records (+id confirmed, -id tentative, 0 not tracked).
 * COLOUR of a painted slot k of image b, in the frames and in the record-driven panel: id = d_ids[b][k];  id == 0: base.color[class]
 * as in "drawing";  otherwise c = palette[(|id| - 1) % npal] (npal 1..32 RGB triples), and for a tentative track (id < 0) every
 * channel (c + 1) >> 1.  Which slots are painted is decided as in "drawing" (flag >= min_flag, class inside [0, ncls) - also for a
 * slot that takes an id colour).  With every id 0 and neither new layer set the call paints what rtm3d_records_draw paints, byte
 * for byte.
 * PAINTER'S ORDER in a frame: first the geometric layers of all slots, last slot first, as in "drawing"; then, with
 * RTM3D_DRAW_LABEL, the labels of all slots, last slot first, per slot the background, then its glyphs left to right.  No label is
 * covered by a box, and slot 0's label ends on top.
 * FONT: 44 glyphs of 5 columns x 7 rows - space, 0-9, A-Z, # ? . % - : / in this order - in a cell of 6 x 8.  rtm3d_draw_font_rows
 * (a HOST function, no device access) gives the seven rows of a character, top row first, 5 low bits per row, bit 4 the LEFT
 * column; it returns non-zero (rows untouched) for a character outside the set - lower case included, which is folded only in
 * names.  The bitmaps are the project's own and live in csrc/draw_font.h alone.  A glyph drawn at scale s = font_scale (1..4)
 * with its top-left pixel at (gx, gy) covers pixel (x, y) iff x >= gx, y >= gy and, with c = (x - gx) / s, r = (y - gy) / s (integer
 * division), c < 5, r < 7 and bit (4 - c) of row r is set: every glyph pixel is an s x s block.  A glyph is ONE primitive: it is
 * not drawn if gx, gy, gx + 5 s - 1 or gy + 7 s - 1 lies outside [-8192, 8192].  The space paints nothing.
 * LABEL TEXT of a slot (rtm3d_draw_label_text, a HOST function, composes the same text by the same code): the fields of the mask
 * label_fields (0..15) in this order, joined by ONE space, an empty field left out with its space:
 *   1  the id: '#' and the decimal digits of |id| % 10000000, '?' instead of '#' for a tentative track (id < 0); empty for id 0;
 *   2  the class name: the bytes of names[class] before the first NUL, 7 at most, a - z drawn as A - Z, any byte outside the set
 *      as '?'; empty for an empty name;
 *   4  the score: two digits and '%': n = (int)((double)[1] * 100.0), 0 if that product is negative or NaN, 99 if it is >= 99;
 *   8  the distance, for a slot with flag 2 only (empty otherwise): n = (int)((double)[29] * 10.0), 0 if the product is negative or
 *      NaN, 9999 if it is >= 9999; the decimal digits of n / 10, '.', the digit n % 10, 'M'.
 *   At most 27 characters.  The two products are single IEEE fp64 operations.  rtm3d_draw_label_text takes the slot as one of flag
 *   2 (the text of another slot is that with bit 8 cleared); it writes the text and a NUL to out[32] and returns non-zero for a
 *   NULL pointer, a label_fields outside 0..15 or a class outside [0, base.ncls).
 * LABEL GEOMETRY (RTM3D_DRAW_LABEL; every painted slot with a text of n >= 1 characters): (x1, y1) = COORD of [20], [21]; if
 * either is BAD the slot has no label.  s = font_scale.  The BACKGROUND is the filled rectangle of the columns x1 .. x1 +
 * (6 n + 1) s - 1 and the 9 s rows top .. top + 9 s - 1, top = y1 - 9 s (above the box), or top = y1 (inside it) when y1 - 9 s < 0;
 * in the slot's COLOUR, opaque.  Glyph i (0 ..) has its top-left pixel at (x1 + s + 6 s i, top + s): one s of padding on every
 * side of the text, one s between the cells' glyphs.  GLYPH COLOUR: black (0, 0, 0) if 299 r + 587 g + 114 b >= 128000 for the
 * background colour (r, g, b), else white (255, 255, 255).  The background and every glyph are separate primitives: the
 * background is not drawn if one of its four extents lies outside [-8192, 8192], a glyph by the rule above, the others are.
 * RTM3D_DRAW_TRACK_BEV: the panels d_bev as for RTM3D_DRAW_BEV (same sizes and mapping), painted from d_state instead of the
 * records; setting both panel bits is refused.  d_state: the tables of "tracking" for B streams of T slots (1..256), stream b for
 * panel b, READ ONLY; may be NULL without this bit.  A slot is drawn iff [0] is >= 1 (and < 2^31; id = (int)[0]): coasting slots -
 * misses [4] > 0, no record of this frame - included.  A slot is TENTATIVE iff hits [3] < 1, that is, iff it was not matched in
 * the frame the table was last updated with: min_hits is not in the table, so the confirmation of step 6 cannot be restated; a
 * coasting track is tentative under step 6 as well (hits 0 < min_hits, once frame > min_hits), a matched one is drawn confirmed
 * here even where step 6 still calls it tentative.  Colour: palette[(id - 1) % npal], halved as above while tentative.  Slots are
 * painted FROM THE LAST TO THE FIRST, per slot in this order, all of thickness 1 and in that colour:
 *   the footprint [7:14] = h w l X Y Z ry: corners, centre and +x midpoint from hl = l / 2, hw = w / 2, c = cos(ry), s = sin(ry)
 *     by the mapping and the corner order of RTM3D_DRAW_BEV, all in fp64 (the table's own values): four outline segments;
 *   the heading mark centre - midpoint;
 *   with vel_horizon > 0 the velocity mark: the segment from the centre to the mapped point x = X + vx * vel_horizon, z = Z + vz *
 *     vel_horizon ([14], [16]; the rounded product, then the rounded sum; u = trunc(bev_w / 2. + x / m), v = trunc(bev_h - z / m));
 *   with label_fields & 1 the id text - '#' or '?' (tentative) and the digits, as field 1 of a label - as glyphs without a
 *     background, glyph i with its top-left pixel at (cu + 6 s i, cv), (cu, cv) the mapped centre; none if the centre is BAD.
 *   A primitive with a BAD coordinate (a state that is not finite) is not drawn, the others of the slot are.
 * bev_fade (0..256): with a value < 256 and either panel layer set, every pixel channel of every panel becomes (px * bev_fade +
 * 128) >> 8 before anything is painted - passing the same panels frame after frame leaves fading trails - and every panel tile
 * is read and written; with 256 a tile nothing touches is neither read nor written, as in "drawing".
 * rtm3d_draw_tracks_default_params: base = rtm3d_draw_default_params (no new layer), a palette of 32 colours of the project's own
 * choosing, label_fields 3, font_scale 1, names "C0" .. "C15", bev_fade 256, vel_horizon 1.
 * rtm3d_records_draw_tracks: one launch per 64 frames, the gather of rtm3d_records_draw (csrc/draw_tracks.hip); stream-ordered, no
 * host synchronisation, no memset / memcpy node, no allocation.  REFUSED before anything is launched, non-zero with the field
 * name in rtm3d_last_error(): everything rtm3d_records_draw refuses, in its words (layers: a mask of the seven bits; d_bev and the
 * panel's size and scale are needed with either panel bit); both panel bits; npal outside 1..32; font_scale outside 1..4;
 * label_fields outside 0..15; RTM3D_DRAW_LABEL with label_fields 0; bev_fade outside 0..256; vel_horizon negative or not finite;
 * a NULL d_ids; with RTM3D_DRAW_TRACK_BEV a NULL d_state or T outside 1..256.                                            */
#define RTM3D_DRAW_LABEL 32
#define RTM3D_DRAW_TRACK_BEV 64
typedef struct rtm3d_draw_tracks_params {
    rtm3d_draw_params base;                         /* as for rtm3d_records_draw; layers may carry the two new bits */
    int npal;
    uint8_t palette[32][3];
    int label_fields, font_scale;
    char names[RTM3D_ENGINE_MAX_CLASSES][8];
    int bev_fade;
    double vel_horizon;
} rtm3d_draw_tracks_params;
int rtm3d_draw_tracks_default_params(rtm3d_draw_tracks_params* p);
int rtm3d_records_draw_tracks(void* stream, int B, int topk, const float* d_rec, const int32_t* d_ids, int T,
                              const double* d_state /* NULL unless RTM3D_DRAW_TRACK_BEV */, uint8_t* const* h_imgs, const int* h_hw,
                              const double* d_K_camera, const rtm3d_draw_tracks_params* params, uint8_t* d_bev);
int rtm3d_draw_font_rows(int ch, uint8_t rows[7]);
int rtm3d_draw_label_text(const rtm3d_draw_tracks_params* p, int id, int cls, float score, float z, char out[32]);

/* ------------------------------------------------------------------ tracking evaluation (csrc/mot_eval.hip)
 * The quality of a tracker on labelled sequences: HOTA and CLEAR-MOT over per-frame similarity matrices of whatever metric (3D
 * IoU, BEV IoU, IoU of the image rectangles: rtm3d_box_overlaps / rtm3d_rect_overlaps).  Added in ABI 9 without changing any
 * existing declaration; nothing calls these unless the caller does.  The host side - label files, the KITTI preprocessing, the
 * closing formulas - is rtm3d_amd/mot_eval.py.  The protocol is restated from the published behaviour of the HOTA / CLEAR
 * evaluation (TrackEval) and of the KITTI tracking benchmark's preprocessing; those programs were not available to compare
 * against, so parity with them is UNPINNED: the contract is the rules written here, and tests/mot_eval_ref.py is written from
 * them.  Everything is fp64, compiled without contraction; "a * b + c" is the rounded product, then the rounded sum; sums run in
 * the order named, left to right; no result depends on the order in which lanes or atomics retire.  EPS = 2.220446049250313e-16.
 *
 * INPUTS.  S sequences, their frames concatenated, F in all: d_seq_start [S + 1] int32, sequence s = frames seq_start[s] ..
 * seq_start[s + 1] - 1 (seq_start[0] = 0, seq_start[S] = F, not decreasing).  Per frame d_ng[f] <= cap_g ground truths and
 * d_nt[f] <= cap_t tracker boxes, 1 <= cap_g, cap_t <= 256 (the limit of rtm3d_tracks_update).  d_gid [F][cap_g], d_tid [F][cap_t]
 * int32: DENSE ids, 0 .. n_gid - 1 / 0 .. n_tid - 1 within each sequence (n_gid, n_tid: the largest count of any sequence; the
 * arrays below are padded to them), an id at most once per frame (the host checks; the device does not).  d_sim [F][cap_g][cap_t]
 * fp64 in [0, 1].  Entries beyond ng / nt are never read.  d_gslot [F][n_gid] / d_tslot [F][n_tid] int32: the slot at which the
 * id stands in the frame, -1 if it is absent (the inverse of d_gid / d_tid, built by the host).
 *
 * ASSIGN, the shared primitive (rtm3d_mot_assign).  For one frame, a score matrix w [cap_g][cap_t] >= 0.  The CANDIDATES are the
 * pairs (g < ng, t < nt) with w > 0 (never NaN).  The match is a matching over candidates - no row and no column twice - with
 * the largest sum of scores; unmatched rows and columns cost nothing; a non-candidate is never matched.  This is step 3b of
 * "tracking" with gain = w.  Where several matchings attain the maximum within the fp64 rounding of the sums, any one may be
 * returned, the same one on every call with the same inputs.  d_match [F][cap_g] int32: the tracker slot, or -1 (also beyond
 * ng).  One wavefront per frame runs shortest augmenting paths (csrc/assign_wave.h, the solver step 3b runs); a frame with ng,
 * nt <= 64 with one column per lane, a larger one with four - the frame's own size decides, not the caps.
 *
 * HOTA (rtm3d_mot_hota), per sequence:
 * 1 ALIGNMENT, for every frame in frame order: rowsum[g] = sum over t < nt of sim[g][t] in t order, colsum[t] = sum over g < ng
 *   in g order; den = (rowsum[g] + colsum[t]) - sim[g][t]; simn = sim[g][t] / den where den > 0, else 0;
 *   potential[gid[g]][tid[t]] += simn - per pair ONE running sum in frame order; gcount[gid] += 1, tcount[tid] += 1 for every id
 *   present in the frame.
 * 2 A[i][j] = potential[i][j] / ((gcount[i] + tcount[j]) - potential[i][j]) - the counts added as integers, then converted - or 0
 *   where that denominator is not positive.
 * 3 per frame: w[g][t] = A[gid[g]][tid[t]] * sim[g][t]; ASSIGN.
 * 4 thresholds a = 0 .. 18 (RTM3D_MOT_ALPHAS of them): alpha_a = 0.05 + a * 0.05; a matched pair COUNTS at a iff
 *   sim >= alpha_a - EPS.
 * 5 per a: TP[a] = counted pairs; FN[a] = sum over frames of ng - counted; FP[a] = sum of nt - counted; loc[a] = the sum of sim
 *   over the counted pairs, ONE running sum in frame order, then ground-truth slot order; mc[a][gid][tid] = the number of frames
 *   in which the pair counted.
 * Device outputs: d_potential [S][n_gid][n_tid] fp64, d_gcount [S][n_gid], d_tcount [S][n_tid] int32, d_match [F][cap_g], d_loc
 * [S][19] fp64 are WRITTEN; d_tp / d_fn / d_fp [S][19] int32 and d_mc [S][19][n_gid][n_tid] int32 are ADDED TO (vector atomics on
 * integers; the caller zeroes them).  Four launches - the sums of every frame; one lane per (gid, tid) pair of a sequence that
 * walks its frames in order (steps 1, 2); one wavefront per frame (3 - 5); one wavefront per sequence for loc - and no host
 * synchronisation, no allocation, no memset / memcpy node.  The closing formulas are the host's (rtm3d_amd/mot_eval.py), per a
 * over all sequences, sums over sequences in sequence order: DetA = TP / max(1, TP + FN + FP), DetRe = TP / max(1, TP + FN),
 * DetPr = TP / max(1, TP + FP); per pair of a sequence assa = mc / max(1, (gcount + tcount) - mc), AssA = sum(mc * assa) /
 * max(1, TP), AssRe with mc / max(1, gcount), AssPr with mc / max(1, tcount) in the place of assa; LocA = loc / max(1, TP), 1.0
 * where TP = 0; HOTA = sqrt(DetA * AssA); every one also as the mean over the 19 thresholds.
 *
 * CLEAR-MOT (rtm3d_mot_clear), per sequence, frames in order with carried state: last[gid] = the tracker id of the ground truth's
 * most recent match, or none; prev[gid] = the tracker id it was matched to in the most recent PROCESSED frame, or none.  thr is
 * the similarity threshold (0.5 in the host's default).  Per frame:
 *   ng == 0: FP += nt, nothing else changes.  nt == 0: FN += ng and idcount[gid] += 1 for every ground truth of the frame;
 *   nothing else changes.  Neither frame is PROCESSED: the carried state, prev included, stays as it is.
 *   otherwise w[g][t] = 1000 * (prev[gid[g]] == tid[t]) + sim[g][t] (1000 + sim, or sim), set to 0 where sim < thr - EPS; ASSIGN.
 *   A matched pair is an identity switch (IDSW += 1) iff last[gid] exists and differs from the matched tid.
 *   idcount[gid] += 1 for every ground truth present, matched[gid] += 1 for the matched ones.  A ground truth whose prev was none
 *   before this frame and is set after it adds 1 to frag[gid].  last is updated for the matched ground truths; prev is cleared
 *   for every id of the sequence, then set for the matched ones.  TP += matched pairs, FN += ng - matched, FP += nt - matched,
 *   simsum += sim of every matched pair: ONE running sum in frame order, then ground-truth slot order.
 * Device outputs: d_match [F][cap_g] and d_simsum [S] fp64 are WRITTEN; d_counts [S][4] int32 = TP, FN, FP, IDSW and d_idcount /
 * d_matched / d_frag [S][n_gid] int32 are ADDED TO (plain adds of the sequence's one wavefront; the caller zeroes them).  One
 * launch, one wavefront per sequence: a frame's scores depend on the previous frame's match, so the frames of a sequence are a
 * chain and S wavefronts are all the parallelism there is.  Host closing formulas: MOTA = (TP - FP - IDSW) / max(1, TP + FN);
 * MOTP = simsum / max(1, TP); Recall = TP / max(1, TP + FN); Precision = TP / max(1, TP + FP); with ratio = matched / idcount
 * over the ids with idcount > 0: MT = ratio > 0.8, PT = ratio >= 0.2 and not MT, ML = the rest; Frag = sum of (frag - 1) over the
 * ids with frag > 0.
 *
 * KITTI PREPROCESSING (host rule, rtm3d_amd/mot_eval.py, optional), per evaluated class C (Car: distractor Van; Pedestrian:
 * distractor Person_sitting; any other class: no distractor), per frame, type comparison ignoring case.  The tracker boxes of type
 * C are ASSIGNed against ALL ground truths of the frame that are not DontCare, rows = ground truths in file order, columns = the
 * tracker boxes in file order, w = sim where sim >= 0.5 - EPS, else 0.  A tracker box is REMOVED if it is matched to a ground
 * truth of the distractor type, or to one of type C with occlusion > 2 or truncation > 0 (the label file's values compared as
 * they are).  An UNMATCHED tracker box is removed if (intersection / its own area) of its image rectangle with any DontCare
 * rectangle of the frame (rtm3d_rect_overlaps, criterion 1) is > 0.5, strictly.  A tracker box matched to any other ground truth
 * stays.  The ground truths KEPT are those of type C with occlusion <= 2 and truncation <= 0.  Then ids are made dense per
 * sequence in order of first appearance (frame order, then file order) and the similarity matrix is cut to the kept rows and
 * columns, both in file order.  Without preprocessing: ground truths = all of type C, tracker boxes = all of type C.
 *
 * rtm3d_mot_workspace_bytes: what d_ws of rtm3d_mot_hota / rtm3d_mot_clear must hold (either; fully rewritten by every call); 0
 * for sizes that would be refused.  Refused before anything is launched, non-zero with the reason in rtm3d_last_error(): S or F
 * < 1, cap_g or cap_t outside 1..256, n_gid or n_tid < 1, S * 19 * n_gid * n_tid beyond 2^31 - 1, a NULL pointer, a thr that is
 * not finite (NaN included); by rtm3d_mot_hota also S > 65535.                                                            */
#define RTM3D_MOT_ALPHAS 19
size_t rtm3d_mot_workspace_bytes(int S, int F, int cap_g, int cap_t, int n_gid, int n_tid);
int rtm3d_mot_assign(void* stream, int F, int cap_g, int cap_t, const int32_t* d_ng, const int32_t* d_nt, const double* d_w,
                     int32_t* d_match);
int rtm3d_mot_hota(void* stream, int S, int F, int cap_g, int cap_t, int n_gid, int n_tid, const int32_t* d_seq_start,
                   const int32_t* d_ng, const int32_t* d_nt, const int32_t* d_gid, const int32_t* d_tid, const int32_t* d_gslot,
                   const int32_t* d_tslot, const double* d_sim, double* d_potential, int32_t* d_gcount, int32_t* d_tcount,
                   int32_t* d_match, int32_t* d_tp, int32_t* d_fn, int32_t* d_fp, double* d_loc, int32_t* d_mc, void* d_ws);
int rtm3d_mot_clear(void* stream, int S, int F, int cap_g, int cap_t, int n_gid, int n_tid, const int32_t* d_seq_start,
                    const int32_t* d_ng, const int32_t* d_nt, const int32_t* d_gid, const int32_t* d_tid, const double* d_sim,
                    double thr, int32_t* d_match, int32_t* d_counts, double* d_simsum, int32_t* d_idcount, int32_t* d_matched,
                    int32_t* d_frag, void* d_ws);

/* ------------------------------------------------------------------ rig fusion (csrc/rig.hip)
 * The C cameras of one vehicle as ONE scene: every camera's kept 3D boxes taken to a common rig frame by the camera's
 * extrinsics, the boxes that several cameras report for one object merged into one, and a map from every camera's record slot
 * to the fused slot, so that a track id given to a fused box finds its way back to each camera's records.  Added in ABI 9
 * without changing any existing declaration; nothing calls these unless the caller does (no plan, engine file or record
 * changes).  The records are READ ONLY.  The rule below is complete: tests/rig_ref.py is written from it.  Everything is fp64,
 * in the operation order written here, compiled without contraction; "a * b + c" means the rounded product, then the rounded
 * sum, and sums associate left to right unless bracketed.  wrap, PI, TWO_PI are those of "tracking"; HALF_PI =
 * 1.5707963267948966.
 *
 * SIZES: R rigs (or R time steps of one rig) of C cameras each.  d_rec [R * C][topk][32] fp32 records, the image of camera c
 * of rig r at index r * C + c.  1 <= C <= 16, 1 <= topk <= 256, C * topk <= 2048, output capacity 1 <= cap <= 256, R >= 1;
 * anything else is refused before a launch.
 * EXTRINSICS: d_ext [R * C][12] fp64 device memory; e = d_ext + 12 * (r * C + c) is the row-major 3 x 4 [R | t] that takes a
 * point of camera c's coordinates to the rig frame - the convention of the tracker's d_ego.
 * RIG FRAME: camera-like, x right, y down, z forward (the frame of a camera whose extrinsic is the identity).  The fused records
 * are therefore records like any camera's: rtm3d_box_overlaps, rtm3d_records_nms3d, rtm3d_tracks_update / _assign and the
 * bird's-eye panels apply to them unchanged.  A caller whose vehicle frame is x forward / z up folds that fixed change of axes
 * into the extrinsics.
 *
 * One call = one frame of every rig, in these steps.
 * 1 CANDIDATES of rig r: the record slots (camera c, slot k) with flag [31] == 2 and (double)[1] >= min_score (a NaN score is
 *   therefore no candidate); class [0], score [1].  The box (h, w, l) = (double)[24:27] is kept as it is.  With (x, y, z, ry) =
 *   (double)[27:31] and the camera's e:
 *     X' = ((e[0] * x + e[1] * y) + e[2] * z) + e[3]      (Y', Z' alike with e[4..7], e[8..11])
 *     ry' = wrap(atan2(-(e[8] * c - e[10] * s), e[0] * c - e[2] * s)),  c = cos(ry), s = sin(ry)
 *   - the heading vector (c, 0, -s) turned with R, as the tracker turns it with the ego motion.  With a pitched or rolled camera
 *   this is an approximation: the box's vertical axis is taken as the rig's (h stays the extent along y), only the heading's
 *   projection into the x-z plane is kept.
 * 2 ORDER the candidates of a rig by score descending - the fp32 compare of [1], so -0 and +0 tie - then by lower camera index,
 *   then by lower slot.
 * 3 CLUSTERS.  linked(i, j) of two candidates holds iff  (cross_only == 0 or camera of i != camera of j)  and  (class_aware == 0
 *   or class of i == class of j, compared as the fp32 values)  and  affinity(box a = the box of j, box b = the box of i) > thresh
 *   (strict; never true for NaN).  The affinity is exactly step 2 of "tracking" on the boxes of step 1 here: metric 0 = BEV IoU,
 *   1 = 3D IoU by the arithmetic of rtm3d_box_overlaps, criterion 0, with the reach shortcut - (ex, ey, ez) = centre a - centre
 *   b, reach = 0.5 * sqrt(w_a * w_a + l_a * l_a) + 0.5 * sqrt(w_b * w_b + l_b * l_b), a pair with ex * ex + ez * ez > reach * reach
 *   has affinity 0 - and metric 2 = -sqrt((ex * ex + ey * ey) + ez * ez).  A box that is not finite (or not positive in h, w, l)
 *   has IoU 0 with everything and a NaN or infinite distance: it links to nothing unless thresh admits 0.
 *   Walk the candidates in the order of step 2.  Candidate i joins the EARLIEST candidate j before it in that order that is a
 *   representative and has linked(i, j); if there is none, i becomes a representative itself.  Members never attract other
 *   candidates: with A-B linked, B-C linked and A-C not linked (A, B, C in this order), B joins A and C is its own
 *   representative.  With cross_only, two boxes of ONE camera can still land in one cluster, each through its link to a
 *   representative of another camera; cross_only only keeps two boxes of one camera from linking to each other.
 * 4 MERGE of a cluster, members m = the representative first, then the other members in the order of step 2:
 *   RTM3D_RIG_MERGE_BEST: the representative's box of step 1.
 *   RTM3D_RIG_MERGE_MEAN: w_m = (double)score of m;  W = sum of w_m;  h, w, l, X, Y, Z each = (sum of w_m * v_m) / W (every sum
 *     starts with the representative's term);  heading: d_m = wrap(ry_m - ry_rep); if d_m > HALF_PI: d_m = d_m - PI, otherwise if
 *     d_m < -HALF_PI: d_m = d_m + PI (a box seen from the other end is the same box);  ry = wrap(ry_rep + (sum of w_m * d_m) / W).
 *     A cluster of one goes through the same arithmetic ((w * v) / w, within a rounding of v), and a cluster whose scores sum to 0
 *     has a box that is not a number: set min_score above 0 where scores of 0 occur.
 *   Class and score of a cluster are the representative's, copied exactly.
 * 5 OUTPUTS, all rewritten in full by every call (no memset is needed):
 *   d_out [R][cap][32] fp32 records: slot s = the s-th representative in the order of step 2, so the output is score-descending
 *     (what the tracker's births rely on).  [0] class  [1] score  [2:24] zero  [24:31] the fused box h w l X Y Z ry rounded to
 *     fp32  [31] = 2.  Slots past the last cluster: 32 zeros.
 *   d_box [R][cap][7] fp64, may be NULL: the fused box before that rounding, zeros in empty slots.
 *   d_info [R][cap][4] int32: the representative's camera, its record slot, the member count (representative included), the bit
 *     mask of the cameras in the cluster (bit c = camera c).  All zero in empty slots.
 *   d_map [R * C][topk] int32, one per record slot: -1 not a candidate; s >= 0 the output slot of its cluster; -2 its cluster did
 *     not fit in cap.
 *   d_n [R][2] int32: clusters written, clusters dropped.  The dropped ones are the last in the order: the lowest scores.
 *
 * rtm3d_rig_default_params: metric 0, thresh 0.1, class_aware 1, cross_only 1, merge RTM3D_RIG_MERGE_MEAN, min_score 0.  There is
 * no multi-camera recording behind these values: they are a choice (a loose BEV IoU, since two cameras' depth errors differ),
 * not a tuning.
 * rtm3d_rig_fuse: three launches - one workgroup per rig for steps 1 and 2 (the keys sorted in LDS), one lane per ordered pair
 * for the linked bits, one workgroup per rig for the scan of step 3 and steps 4, 5 - through d_ws, rtm3d_rig_workspace_bytes(R,
 * C, topk) bytes, whatever it holds before the call (0 for sizes the call refuses).  Stream-ordered: no host synchronisation, no
 * memset / memcpy node, no allocation.  No result depends on the order in which lanes retire: two calls on the same inputs are
 * bit-identical, and a call with R rigs equals R calls with one.  Refused before anything is launched, non-zero with the reason in
 * rtm3d_last_error(): sizes outside the ranges above, a NULL d_rec / d_ext / params / d_out / d_info / d_map / d_n / d_ws, metric
 * outside 0..2, merge outside 0..1, NaN thresh or min_score.
 * rtm3d_rig_scatter_ids: d_ids_cam [R * C][topk] = d_map >= 0 ? d_ids_rig [r][d_map] : 0 with d_ids_rig [R][cap] - the ids the
 * tracker returns for the fused records (B = R, topk = cap) taken back to each camera's slots, the array
 * rtm3d_records_draw_tracks and the users of the per-camera records expect.  One launch; refused alike: sizes, a NULL pointer. */
#define RTM3D_RIG_MERGE_BEST 0
#define RTM3D_RIG_MERGE_MEAN 1
typedef struct rtm3d_rig_params {
    int metric, class_aware, cross_only, merge;
    double thresh, min_score;
} rtm3d_rig_params;
int rtm3d_rig_default_params(rtm3d_rig_params* p);
size_t rtm3d_rig_workspace_bytes(int R, int C, int topk);
int rtm3d_rig_fuse(void* stream, int R, int C, int topk, int cap, const float* d_rec, const double* d_ext,
                   const rtm3d_rig_params* params, float* d_out, double* d_box, int32_t* d_info, int32_t* d_map, int32_t* d_n,
                   void* d_ws);
int rtm3d_rig_scatter_ids(void* stream, int R, int C, int topk, int cap, const int32_t* d_map, const int32_t* d_ids_rig,
                          int32_t* d_ids_cam);

/* ---- validation loss ------------------------------------------------------------------------------------------------
 * The number the reference selects checkpoints by (train.py:61-81): KITTI label rows -> the targets of
 * datasets/dataset_reader.py:215-291 (utils/data_utils.py:7-18, 97-141) -> the loss of models/rtm3d_loss.py:268-340
 * (models/nets/module.py:41-68, utils/model_utils.py:10-14).  This block is the forward value; its gradient with respect to the
 * logits is the next block, "loss gradient".
 *
 * INPUT.  N objects, sorted by image: d_obj [N][RTM3D_LOSS_ROW] fp64, one row per object
 *   [0] img_id, 0 <= img_id < B, non-decreasing      [1] cls: the index into DATASET.OBJs, or -1, which sets mask = 0
 *   [2] noise (0 / 1)      [3:7] bbox x1 y1 x2 y2 in network-input pixels (after the caller's resize and letterbox), x2 >= x1 and
 *   y2 >= y1 (the caller's to ensure: the radius of a reversed box is not defined; the Python wrapper refuses it)
 *   [7:10] dimension h w l      [10:13] location, the KITTI bottom centre      [13] Ry      [14] sin(Ry)  [15] cos(Ry) as the
 *   HOST computed them: the device's fp64 sine is not every host's to the last bit, and the table below is defined bit for bit
 *   [16] mask_3d: 0 / 1 supplied by the caller, or -1 = derive it      [17] reserved, 0
 * d_K [B][9] fp64, one row-major K per image, in input pixels.  d_img_start [B + 1] int32: the objects of image b are the rows
 * d_img_start[b] .. d_img_start[b + 1] - 1.
 * Class mapping (the host's work, _transform_obj_label, dataset_reader.py:197-213): a type in DATASET.OBJs is one row of its
 * class, noise 0; a type listed in DATASET.RELATE_OBJs[k] becomes one NOISE row of class k per list that contains it (with the
 * defaults, Person_sitting becomes two rows); everything else becomes one row with cls = -1.
 *
 * PER OBJECT (the table d_table [N][RTM3D_LOSS_TABLE] fp64): fp64, the operation order written here, no contraction; sums and
 * products associate left to right unless bracketed; ds = MODEL.DOWN_SAMPLE; trunc rounds toward zero as astype(long) does.
 *   x1, y1, x2, y2 = bbox / ds;  cx = (x1 + x2) / 2, cy = (y1 + y2) / 2;  m_proj = trunc(centre);  m_off = centre - m_proj
 *   radius (_compute_gaussian_radius, min_overlap mo = 0.7):  hh = ceil(y2 - y1), ww = ceil(x2 - x1)
 *     b1 = hh + ww                c1 = ww * hh * (1 - mo) / (1 + mo)    r1 = (b1 + sqrt(b1 * b1 - 4 * c1)) / 2
 *     b2 = 2 * (hh + ww)          c2 = (1 - mo) * ww * hh               r2 = (b2 + sqrt(b2 * b2 - 16 * c2)) / 2
 *     b3 = (-2 * mo) * (hh + ww)  c3 = (mo - 1) * ww * hh               r3 = (b3 + sqrt(b3 * b3 - (4 * (4 * mo)) * c3)) / 2
 *     r = min(r1, r2, r3);  sigma = (2 * r + 1) / 6;  R = ceil(r);  inv = 1 / (2 * (sigma * sigma))
 *     Only DATASET.GAUSSIAN_GEN_TYPE = 'dynamic_radius' exists here ('dynamic_sigma' cannot run in the reference either).
 *   vertices: k = K with its first two rows divided by ds;  s = sin(Ry), c = cos(Ry), each set to 0 where its magnitude is
 *     below 1e-3 (rotation_matrix);  the 8 corners are csrc/box_project.h's box_project_corner of x = [s, c, l, h, w, X, Y - h / 2,
 *     Z] - corner j = 4 i_x + 2 i_y + i_z with sign +1 for a 0 bit, (u, v) = (k[0:3] . P, k[3:6] . P) / (k[6:9] . P + 1e-6)
 *     v_proj = trunc(v);  v_off = v - v_proj;  v_coor_off = v - centre;  v_mask = v_proj inside [0, W) x [0, H)
 *   mask_3d: the caller's, or "all eight corners have camera depth ((-s * l / 2) * sx + (c * w / 2) * sz) + Z > 0".  PARITY
 *     UNPINNED: the reference takes this mask from a KITTI devkit module that its tree does not contain.
 *   mask = cls >= 0 (and img_id inside 0 .. B - 1: a row of no image takes no part).
 * Table columns: 0 img  1 cls  2 mask  3 noise  4 mask_3d  5 m_proj inside the map  6:8 centre  8:10 m_proj  10:12 m_off  12 r
 *   13 sigma  14 R  15 inv  16:32 vertices [8][2]  32:48 v_proj  48:64 v_off  64:80 v_coor_off  80:88 v_mask.
 *
 * HEAT-MAP TARGET m_hm[b][c][y][x] = the maximum over the objects i of image b with mask = 1, cls = c, |x - mx| <= R and
 * |y - my| <= R (the full square, no circular cut) of g_i = exp(-((dx * dx + dy * dy) * inv)) in fp64, replaced by 0.9999 at
 * the centre of a noise object; 0 where no object reaches; rounded to fp32 once.  The centre of a non-noise object is therefore
 * exactly 1.0f, which the focal loss's target.eq(1) depends on.  An object whose centre lies outside the map still paints the
 * cells its square reaches.
 *
 * LOSS.  Element terms fp32 as in the reference, every sum fp64 in an order that depends on the sizes only.
 *   p = clamp(1 / (1 + expf(-x)), 1e-4f, 0.9999f) of the heat-map logit x (a NaN stays a NaN);  t = the target
 *   t == 1: pos += logf(p) * (1 - p)^alpha, num_pos += 1;   t < 1: neg += (logf(1 - p) * p^alpha) * (1 - t)^beta
 *   alpha = 2 and beta = 4 are squares ((v * v) * (v * v)), other values powf.  num_pos counts the whole batch.
 *   main = -(pos + neg) / num_pos, or -neg when num_pos = 0.
 *   The three L1 terms are means over their selections (rtm3d_loss.py:300-329), each |prediction - (float)target| in fp32:
 *     ver_coor   the raw 16 ver_coor logits at m_proj, channels 2 j, 2 j + 1 against v_coor_off of vertex j, for the objects with
 *                mask and not noise and mask_3d, of those the vertices with v_mask
 *     vertex_off sigmoid of the 2 v_off logits at v_proj against v_off, the same objects and vertices
 *     main_off   sigmoid of the 2 m_off logits at m_proj against m_off, for the objects with mask and not noise
 *   An empty selection gives NaN (F.l1_loss of nothing; the reference's test_epoch stops on it).  An object with mask and not
 *   noise whose m_proj lies outside the map - the reference would raise or wrap there - is left out of the three terms and
 *   counted in n_outside.
 *   d_out [5] fp32: W_MKF * main, W_VFM * ver_coor, W_M_OFF * main_off, W_V_OFF * vertex_off (each term rounded to fp32, times
 *   the fp32 weight) and their fp32 sum in this order.  d_counts [5] int32: num_pos, the vertices of ver_coor, the vertices of
 *   vertex_off, the objects of main_off, n_outside.  NaN or infinite logits propagate into the result; nothing faults on them.
 *
 * rtm3d_loss_objects: one lane per object, writes d_table.  rtm3d_loss_heatmap: m_hm [B][C][H][W] fp32 from the table, for
 * inspection and tests - rtm3d_loss_eval never writes the map: a workgroup takes an image and a band of rows, stages that
 * image's objects in LDS in chunks of 128 (no cap on the objects of an image), forms each cell's target as it reads the logit
 * (16 bytes per lane when W % 4 == 0 and d_hm is 16-byte aligned) and leaves one fp64 triple (pos, neg, num_pos) in its own
 * slot of d_ws (the byte count: rtm3d_loss_workspace_bytes); one wave then adds the slots - lane l the slots l, l + 64, ... in
 * index order, the lanes by a fixed butterfly - gathers the regression logits, writes d_out / d_counts and, with d_accum
 * [2] fp64 not NULL, adds total * B and B into it (test_epoch's mloss and num).  No atomics: two calls on the same inputs are
 * bit-identical.  d_ws and d_accum belong to one stream at a time (d_accum is updated by a plain read-modify-write).  d_ver_coor [B][16][H][W], d_m_off [B][2][H][W], d_v_off [B][2][H][W], d_hm [B][C][H][W]: the four fp32 logit
 * maps.  H, W must be those the table was built with.  All stream-ordered without host synchronisation, except
 * rtm3d_loss_accum_read, which copies d_accum to h_sum_count [2] and waits for the stream; rtm3d_loss_accum_reset zeroes it.
 * Refused before a launch, non-zero with the reason in rtm3d_last_error: B or C outside 1..65535, H, W < 1, N outside
 * 0..RTM3D_LOSS_MAX_OBJECTS, a NULL pointer, alpha or beta outside (0, 64], a NaN weight, down_sample outside (0, 1e6]. */
#define RTM3D_LOSS_ROW 18
#define RTM3D_LOSS_TABLE 88
#define RTM3D_LOSS_MAX_OBJECTS (1 << 20)
typedef struct rtm3d_loss_params {
    float alpha, beta;              /* MODEL.FOCAL_LOSS_ALPHA, MODEL.FOCAL_LOSS_BEDA */
    float weight[4];                /* TRAINING.W_MKF, W_VFM, W_M_OFF, W_V_OFF */
} rtm3d_loss_params;
int rtm3d_loss_objects(void* stream, int N, int B, const double* d_obj, const double* d_K, double down_sample, int H, int W,
                       double* d_table);
int rtm3d_loss_heatmap(void* stream, int B, int C, int H, int W, const int32_t* d_img_start, const double* d_table, int N,
                       float* d_hm);
size_t rtm3d_loss_workspace_bytes(int B, int C, int H, int W);
int rtm3d_loss_eval(void* stream, int B, int C, int H, int W, const float* d_hm, const float* d_ver_coor, const float* d_m_off,
                    const float* d_v_off, const int32_t* d_img_start, const double* d_table, int N,
                    const rtm3d_loss_params* params, void* d_ws, float* d_out, int32_t* d_counts, double* d_accum);
int rtm3d_loss_accum_reset(void* stream, double* d_accum);
int rtm3d_loss_accum_read(void* stream, const double* d_accum, double* h_sum_count);

/* ---- loss gradient --------------------------------------------------------------------------------------------------
 * The gradient of total (d_out[4] of rtm3d_loss_eval) with respect to every element of the four fp32 logit maps, times an
 * upstream scalar u (d_upstream: one fp32 on the device, NULL = 1): what loss.backward() of the reference's train_epoch leaves
 * in the logits.  Element terms are fp32 in the operation order written here (no contraction, brackets as shown, otherwise left
 * to right); there is no fp64 sum.  The symbols are those of "validation loss".
 *
 * HEAT MAP, every cell.  t = the target, formed exactly as the forward forms it (0.9999 at a noise centre, the test t == 1 on
 * the fp32 value: where a huge Gaussian rounds a neighbour to 1.0f, that cell is a positive here too).
 *   s = 1 / (1 + expf(-x));  p = clamp(s, 1e-4f, 0.9999f);  in = (s >= 1e-4f) && (s <= 0.9999f), the bounds inclusive as in the
 *   backward of torch's clamp;  q = 1 - p
 *   t == 1:  dp = q^alpha / p - (alpha * q^(alpha - 1)) * logf(p)
 *   t <  1:  dp = (-(p^alpha) / q + (alpha * p^(alpha - 1)) * logf(q)) * (1 - t)^beta
 *   alpha = 2 and beta = 4: v^alpha = v * v, v^(alpha - 1) = v, v^beta = (v * v) * (v * v); other values powf(v, alpha),
 *   powf(v, alpha - 1.0f), powf(v, beta)
 *   k = -((u * W_MKF) / (float)max(num_pos, 1));   g = (k * (in ? dp : 0)) * (s * (1 - s))
 *   num_pos is d_counts[0], what the forward left on the device - not recomputed.  A NaN logit gives a NaN in its own cell only
 *   (0 * NaN); +-inf and saturated logits give exactly 0 (of either sign).
 * REGRESSION MAPS.  sign(d) = 1, -1 or +0 for d > 0, d < 0, d == 0, and d itself for a NaN (torch's sign gives 0 there: a NaN
 * logit would go unseen).  n_* are d_counts[1], [2], [3].  The selections are the forward's, object by object and vertex by vertex:
 *   ver_coor   channels 2 j + e at m_proj:   sign(x - (float)v_coor_off) * k_vc,                  k_vc = (u * W_VFM) / (2.0f * n_ver_coor)
 *   main_off   channels e at m_proj:         (sign(s - (float)m_off) * (s * (1 - s))) * k_mo,     k_mo = (u * W_M_OFF) / (2.0f * n_main_off)
 *   vertex_off channels e at v_proj:         (sign(s - (float)v_off) * (s * (1 - s))) * k_vo,     k_vo = (u * W_V_OFF) / (2.0f * n_vertex_off)
 *   with s = (float)(1 / (1 + exp(-(double)x))) here: the sigmoid through fp64, rounded to fp32 once.  The contributions to one
 *   element differ in their signs only, so whether a run of them cancels to exactly zero hangs on the last bit of s; an expf
 *   differs from library to library in that bit, this value does not (measured: one element of the 150-object test case was an
 *   ulp-sized residue on the device and 0 in numpy with expf).  Every element of the three maps starts as +0.0f and the contributions to it are
 *   added in fp32 in rising object order, then rising vertex order (two objects on one m_proj cell, several vertices that
 *   truncate to one v_proj cell); an element nothing contributes to is +0.0f.  An object counted in n_outside contributes
 *   nothing; an empty selection contributes nothing - its forward item is NaN, the maps stay finite, as autograd leaves them.
 * Every element of every requested output is written: the caller need not clear them.  No floating-point atomics; two calls on
 * the same inputs are bit-identical.
 *
 * rtm3d_loss_grad: two launches, stream-ordered, no host synchronisation, no workspace.  The dense pass has the forward's
 * decomposition (a workgroup per image and band of rows, the image's objects in LDS in chunks of 128; 16 bytes per lane in and
 * out when W % 4 == 0 and d_hm and d_g_hm are 16-byte aligned, cell by cell otherwise), reads each logit and writes its gradient,
 * and clears its band of the 20 regression channels (16-byte stores under the same condition per map).  The sparse pass runs
 * behind it: a workgroup per image takes the image's objects 64 at a time, puts every contribution's element and value in LDS,
 * and the first contribution to an element within the 64 reads the element, adds the others in order and writes it - one writer
 * per element, the groups of 64 one after the other; an image's objects are the rows d_img_start gives it (their table image
 * must be that image).  d_counts [5]: rtm3d_loss_eval's, of the same inputs, read on the device.  Any of the four outputs may be
 * NULL: not wanted, not computed.  Refused before a launch with the reason in rtm3d_last_error: what rtm3d_loss_eval refuses
 * of sizes, pointers and parameters, 16 * H * W beyond an int index, a NULL d_counts, all four outputs NULL, an output pointer
 * equal to an input pointer.  Second derivatives do not exist. */
int rtm3d_loss_grad(void* stream, int B, int C, int H, int W, const float* d_hm, const float* d_ver_coor, const float* d_m_off,
                    const float* d_v_off, const int32_t* d_img_start, const double* d_table, int N, const rtm3d_loss_params* params,
                    const int32_t* d_counts, const float* d_upstream, float* d_g_hm, float* d_g_ver_coor, float* d_g_m_off,
                    float* d_g_v_off);

/* ------------------------------------------------------------------ training augmentation (csrc/augment.hip, csrc/philox.h)
 * The front of the chain uint8 frames -> network input -> logits -> loss -> gradient: the reference's TrainAugmentation
 * (preprocess/data_preprocess.py: RandomBrightnessContrast, GaussNoise, RemoveBadBBox, Resize, RandomAffine(range (1, 1.2),
 * offset 0), RandomMirror), then _apply_padding and Normalize, for B packed uint8 (h, w, 3) frames at once.  The pixels are made
 * here; the labels move in step on the host (rtm3d_amd/augment.py).  One interior launch per chunk of 32 frames, then one border
 * launch per chunk, descriptors by value, stream-ordered, no host synchronisation; the canvas is written directly, no
 * intermediate image exists.  Added in ABI 9 without changing any existing declaration.
 *
 * THE RULE is "the reference's photometric steps applied to the SOURCE frame, then ONE bilinear resample through the composed
 * Resize, RandomAffine and RandomMirror map, then letterbox and normalise".  One interpolation where the reference does two
 * (cv2.resize, then cv2.warpAffine) is a deliberate deviation: a second resampling only blurs.  Integers only (int64 where
 * stated, otherwise int32; >> is arithmetic); tests/augment_ref.py restates it in numpy.  Frame of h x w pixels, source byte v
 * at source pixel p = j * w + i (column i, row j), channel c:
 *   BRIGHTNESS / CONTRAST   L = clamp((v * alpha_q + beta_q) >> 16, 0, 255), the product and sum in int64.  alpha_q =
 *     round(alpha * 65536), beta_q = round(beta * 255 * 65536): albumentations' uint8 table with brightness_by_max.  The
 *     identity is alpha_q = 65536, beta_q = 0.
 *   NOISE   sigma_q == 0: a = L, nothing is drawn.  Otherwise r[0..3] = Philox4x32-10 of counter (p, 0, 0, 0) and key (seed_lo,
 *     seed_hi);  n = (T[r[c] >> 20] * sigma_q + 32768) >> 16;  a = clamp(L + n, 0, 255).  T is plain data, 4096 int16 on the
 *     device, T[k] = round(1024 * Phi^-1((k + 0.5) / 4096)) (Phi the standard normal distribution function); sigma_q =
 *     round(sigma * 64).  rtm3d_augment_noise_table builds T on the host in fp64 with an inverse of its own (Newton steps on
 *     erfc); no entry is nearer than 2.8e-5 to a rounding tie, so any sound fp64 inverse gives the same table.  The largest
 *     entry is 3756: the noise is cut off at 3.67 sigma.  The noise belongs to the source pixel, not to the canvas pixel: the
 *     taps of neighbouring canvas pixels that share a source pixel share its noise.
 *   GEOMETRY   canvas pixel (X, Y) inside the placed rectangle x0 <= X < x0 + rw, y0 <= Y < y0 + rh;  x = X - x0, y = Y - y0.
 *     sx = (x * ax + bx) >> 16,  sy = (y * ay + by) >> 16  (int64): the source position in 1/32 pixel, integer coordinates are
 *     pixel centres.  OUT if sx <= -32 or sx >= 32 * w or sy <= -32 or sy >= 32 * h: the pixel is fill[c].  Otherwise sx is
 *     clamped to [0, 32 * (w - 1)] and sy to [0, 32 * (h - 1)] (edge replication, as cv2.resize does) and the remap rule of
 *     "lens undistortion" is applied to the four values a: ix = sx >> 5, fx = sx & 31, iy = sy >> 5, fy = sy & 31,
 *     out = ((32-fx)*(32-fy)*a(ix,iy) + fx*(32-fy)*a(ix+1,iy) + (32-fx)*fy*a(ix,iy+1) + fx*fy*a(ix+1,iy+1) + 512) >> 10.
 *     A tap of weight 0 is not read (after the clamp those are the only taps that can lie outside the frame).
 *   BORDER   per channel the rw * rh bytes written into the rectangle are summed as integers (the order does not matter);
 *     the pad colour is sum / (rw * rh) truncated, as rtm3d_preprocess defines it; canvas pixels outside the rectangle take it.
 *   NORMALISE   out_mode 0 and 1 put every canvas byte through the fp32 / fp16 table of rtm3d_normalize_luts.
 * out_mode 0: d_out = fp32 NCHW (B, 3, H, W).  out_mode 1: d_out = the plan's fp16 NHWC4 input tensor
 *   [B][H + 2 * out_border][W + 2 * out_border][4], 4th channel 0, the border itself not written - the contract of
 *   rtm3d_preprocess_batch out_mode 1 (rtm3d_input_tensor, rtm3d_forward with d_in == NULL).  out_mode 2: d_out = packed uint8
 *   (B, H, W, 3) canvases at any byte address, exactly B * H * W * 3 bytes written (for inspection, drawing, JPEG encoding).
 *
 * rtm3d_augment_geometry (HOST, no device access): fills h, w, the rectangle and ax, bx, ay, by of *out from a frame's
 * rtm3d_frame_geom - x0 = pad_w, y0 = pad_h, the rectangle = the frame after Resize, centred - and the draw of the affine and the
 * mirror; every other field of *out is left as it is.  The composed map of a rectangle column x to a source column:
 *   no mirror xm = x, mirror xm = rw - 1 - x;   xr = (xm - off_x) / scale  (the affine is dst = scale * src + offset, in the
 *   pixels of the resized frame);   xs = (xr + 0.5) * w / rw - 0.5  (the Resize, pixel centres);   rows alike, never mirrored.
 * It is evaluated in fp64 in this order, every line left to right as written, compiled without contraction:
 *   r = (double)w / (double)rw;   g = r / scale;   m0 = mirror ? (double)(rw - 1) : 0.0;
 *   c = ((m0 - off_x) / scale + 0.5) * r - 0.5;   a = mirror ? -g : g;
 *   ax = (int64)floor(a * 2097152.0 + 0.5);   bx = (int64)floor(c * 2097152.0 + 0.5) + 32768
 * (2097152 = 32 * 65536; the + 32768 is the round-to-nearest of the >> 16, folded into bx); ay, by from h, rh, off_y with mirror
 * = 0.  With scale 1, offsets 0, no mirror and rw == w this is ax = 2097152, bx = 32768: sx = 32 * x, the identity.  Refused: a
 * NULL pointer, a side < 1, a scale that is not finite and > 0, an offset that is not finite, a coefficient beyond int64's 2^62.
 *
 * rtm3d_frames_augment_plan (HOST): the schedule rtm3d_frames_augment gives a batch - the launcher calls the same code;
 * out[(B + 31) / 32] receives one entry per chunk.  A canvas row is cut into runs of px_per_thread consecutive pixels that
 * begin at X = 4 * k - shift, shift = out_border & 3 in out_mode 1 (so that a run is 32 aligned bytes of the NHWC4 tensor) and
 * 0 otherwise.  Interior launch: grid (grid_x, count) x threads; thread t = block * threads + lane of grid row i takes run
 * t % runs_per_row of rectangle row t / runs_per_row of frame first + i, where runs_per_row is the number of runs that meet
 * the columns of the rectangle, and idles when t >= rh * runs_per_row; runs is the largest such product of the chunk.  Border
 * launch: grid (border_grid_x, count) x threads, grid-striding over the H * border_runs_per_row runs of the whole canvas and
 * writing their pixels outside the rectangle; border_grid_x = 0 and no launch when every rectangle of the chunk is its canvas.
 * rtm3d_frames_augment_check (HOST): every refusal of rtm3d_frames_augment, without a launch.  REFUSED, for the whole batch
 * before the first memset or launch, the message naming the frame: a NULL pointer (source, destination, noise table, channel
 * sums, the normalisation table of the mode); a side of a frame or of the canvas < 1 or > 16384; a rectangle with a side < 1 or
 * one that leaves the canvas; sigma_q < 0 or > 65535; |alpha_q| > 2^24; |beta_q| > 2^31 - 2^24; |ax| or |ay| >= 2^40, |bx| or
 * |by| >= 2^56; reserved != 0; out_border < 0 in out_mode 1; an out_mode 2 destination that overlaps a source; an unknown mode.
 *
 * Kernel shape: a thread makes the (up to) 4 pixels of its run and stores them as 2 x 16 B (mode 1), 16 B per plane (mode 0,
 * where the addresses allow it) or through the shared run store of packed RGB (mode 2, csrc/rgb_runs.h); channel sums are
 * reduced within the wave, then the workgroup issues one 64-bit integer atomic per channel.  No float atomics: two calls on the
 * same inputs give the same bytes, and a frame's bytes do not depend on its place in the batch.
 *
 * OUT OF SCOPE: the mosaic path (IS_MOSAIC, RandomAffine2D with rotation and shear, HSV jitter) and PhotometricDistort; parity
 * of pixels with OpenCV or albumentations - both are absent here, the rule above is a restatement that differs by design (one
 * interpolation, 5-bit weights, integer noise cut off at 3.67 sigma); an optimiser and a training loop; a C engine entry point;
 * drawing the parameters on the device.                                                                                  */
typedef struct rtm3d_augment_frame {
    int h, w;                              /* the source frame */
    int x0, y0, rw, rh;                    /* the placed rectangle on the canvas */
    int32_t alpha_q, beta_q;               /* brightness / contrast; identity 65536, 0 */
    int32_t sigma_q;                       /* noise, round(sigma * 64); 0 = none */
    uint32_t seed_lo, seed_hi;             /* the Philox key */
    uint8_t fill[3];                       /* the colour of an OUT pixel */
    uint8_t reserved;                      /* 0 */
    int64_t ax, bx, ay, by;                /* rectangle pixel -> source position, 1/32 pixel << 16 */
} rtm3d_augment_frame;
typedef struct rtm3d_augment_plan {
    int first, count;                      /* frames first .. first + count - 1 */
    int px_per_thread;                     /* 4 consecutive canvas pixels of one row */
    int threads;                           /* per workgroup */
    int shift;                             /* a run begins at X = 4 * k - shift */
    int runs;                              /* interior thread runs of the chunk's largest rectangle */
    int grid_x, grid_y;                    /* interior launch */
    int border_runs_per_row;               /* runs that meet the W columns of a canvas row */
    int border_grid_x;                     /* border launch: grid (border_grid_x, count); 0 = no launch */
} rtm3d_augment_plan;
int rtm3d_augment_noise_table(int16_t out[4096]);
int rtm3d_augment_geometry(const rtm3d_frame_geom* geom, double scale, double off_x, double off_y, int flip, rtm3d_augment_frame* out);
int rtm3d_frames_augment_plan(int B, const rtm3d_augment_frame* h_frames, int out_mode, int H, int W, int out_border,
                              rtm3d_augment_plan* out);
int rtm3d_frames_augment_check(int B, const uint8_t* const* h_src, const rtm3d_augment_frame* h_frames, const void* d_out,
                               int out_mode, int H, int W, int out_border, const int16_t* d_noise_table, const float* d_lut,
                               const void* d_lut16, const unsigned long long* d_sums);
/* h_src[B]: HOST array of DEVICE pointers to packed uint8 (h, w, 3) frames at any byte address; h_frames[B]: HOST descriptors;
 * d_noise_table: T on the device; d_lut / d_lut16: the tables of rtm3d_normalize_luts on the device (d_lut for out_mode 0,
 * d_lut16 for out_mode 1, neither for out_mode 2); d_sums: B * 3 uint64 of device scratch (cleared here, on the stream).  */
int rtm3d_frames_augment(void* stream, int B, const uint8_t* const* h_src, const rtm3d_augment_frame* h_frames, void* d_out,
                         int out_mode, int H, int W, int out_border, const int16_t* d_noise_table, const float* d_lut,
                         const void* d_lut16, unsigned long long* d_sums);

/* ---- optimiser step (rtm3d_amd/optim.py): Adamax, an optional weight EMA and a non-finite-loss guard in one launch ------------
 * The line after loss.backward() of a training loop: the reference's solver.step (torch.optim.Adamax, one parameter group per
 * parameter) as one streaming pass over every parameter of the model.  "Solver" elsewhere in this header is the L-BFGS-B 3D fit.
 *
 * THE RULE, per fp32 element with gradient g, parameter p, first moment m and infinity norm u.  Every operation is its own
 * correctly rounded fp32 operation (no FMA contraction: the translation unit is built with -ffp-contract=off; the quotient is the
 * IEEE quotient), denormals are kept, and numpy restates it operation by operation (tests/optim_ref.py):
 *     g1 = g + wd * p                        only when the element's class has wd != 0; otherwise g1 = g
 *     m1 = m + w * (g1 - m)                  when w < 0.5;  otherwise  m1 = g1 - (g1 - m) * (1.0f - w)     [torch's two lerp branches]
 *     a  = u * beta2,  b = |g1| + eps
 *     u1 = a if (a > b or a is NaN) else b   [torch.maximum: a NaN operand gives NaN; fmaxf would return the other operand]
 *     p1 = p + nclr * (m1 / u1)
 *     e1 = e * d + omd * p1                  only where an EMA is kept
 * Which NaN a NaN result is (sign, payload) is not part of the rule.  An element whose gradient is NaN or +-Inf becomes non-finite
 * (Inf: m1 = u1 = Inf, the quotient NaN); its neighbours are untouched.  The scalars are formed ON THE HOST and passed by value:
 *     w = (float)(1 - beta1), beta2 = (float)beta2, eps = (float)eps, wd = (float)weight_decay      [fp64 first, rounded once]
 *     nclr = (float)(-(lr / (1 - beta1 ** t)))      t = the number of this step, 1, 2, ...; fp64 as torch forms clr
 *     d = (float)(decay * (1 - exp(-n / 2000))),  omd = (float)(1.0 - that fp64 value)           n = the EMA's update count
 * Elements with the same (lr, weight_decay) form a HYPER CLASS {nclr, wd}; a launch takes RTM3D_OPTIM_MAX_CLASSES.
 * torch's CPU kernels contract some of these pairs to FMA, so the rule is torch's within rounding, not to the last bit
 * (tests/test_optim_cpu.py holds it within max(4 x torch's own fp32-vs-fp64 distance, 4 ulp) of torch's fp64 trajectory).
 *
 * SEGMENTS.  The host describes N segments (rtm3d_optim_segment): n fp32 elements at DEVICE addresses that are multiples of 4,
 * a class and a kind -
 *     RTM3D_OPTIM_UPDATE_EMA (0)  p, g, m, u, e: the update, then the EMA line on p1
 *     RTM3D_OPTIM_UPDATE     (1)  p, g, m, u:    the update alone
 *     RTM3D_OPTIM_EMA        (2)  p, e:          the EMA line alone on p as it is, p is only read (a floating-point buffer of the
 *                                                model, e.g. BatchNorm's running statistics)
 * Pointers a kind does not use are ignored.  rtm3d_optim_plan (HOST) checks the segments and writes the two tables the kernel
 * walks: the segment table (the N descriptors as given) and the chunk table, one rtm3d_optim_chunk {segment, index} per run of
 * RTM3D_OPTIM_CHUNK elements index * CHUNK .. of a segment, segments in order, a segment's chunks in rising index; the last chunk
 * of a segment is short, a chunk never crosses a segment, a segment of 0 elements has no chunk, and every element of every
 * segment lies in exactly one chunk.  The caller copies both tables to the device (8-byte aligned).  REFUSED, by code
 * (RTM3D_OPTIM_E_*, the message in rtm3d_last_error): a NULL argument or a NULL pointer a kind uses (E_NULL); N < 1 (E_COUNT);
 * n < 0 or n > 2^40 (E_SIZE); a class outside 0 .. 15 (E_CLASS); an unknown kind (E_KIND); an address that is no multiple of 4 (E_ALIGN);
 * any two used ranges of any segments that overlap (E_OVERLAP); more than 2^31 - 1 chunks (E_TOO_MANY).
 * rtm3d_optim_table_bytes (HOST): the bytes of the two tables and the chunk count for N segment sizes.
 *
 * rtm3d_optim_step: ONE launch, no synchronisation, no atomics, no workspace.  min(chunks, compute units) workgroups of 1024
 * threads (16 waves per compute unit) stride over the chunk table; a chunk whose pointers are all multiples of 16 moves 16 B per lane and access (its last
 * n & 3 elements singly), any other chunk one element per lane and access - parameters are the caller's storage and may sit
 * at any multiple of 4.  Gradients are read with non-temporal loads.  Each element has one writer: two runs on equal inputs
 * leave equal bytes.
 * GUARD: with d_loss != NULL the launch reads that fp32 value first; if it is NaN or +-Inf NO byte of p, m, u, e is written and
 * one lane adds 1 to *d_skipped (an ordinary load and store: the counter belongs to one stream).  The host's counts t and n
 * advance all the same - that is what lets it form the scalars without reading anything back.  With d_loss == NULL the update
 * always applies.  DEVIATION from the reference, which tests torch.isfinite(loss) on the host (one synchronisation per step) and
 * ends training: here the step is skipped and counted, and the caller reads the counter when it wants to.
 *
 * OUT OF SCOPE: the network's backward pass, a training loop, gradient clipping, loss scaling, SGD / Adam, an all-reduce (the
 * gradient arena of rtm3d_amd/optim.py is one flat tensor so that one collective can reduce it), graph capture of the step, a C
 * engine entry point.                                                                                                        */
#define RTM3D_OPTIM_CHUNK 4096
#define RTM3D_OPTIM_MAX_CLASSES 16
enum { RTM3D_OPTIM_UPDATE_EMA = 0, RTM3D_OPTIM_UPDATE = 1, RTM3D_OPTIM_EMA = 2 };
enum { RTM3D_OPTIM_E_NULL = 1, RTM3D_OPTIM_E_COUNT = 2, RTM3D_OPTIM_E_SIZE = 3, RTM3D_OPTIM_E_CLASS = 4, RTM3D_OPTIM_E_KIND = 5,
       RTM3D_OPTIM_E_ALIGN = 6, RTM3D_OPTIM_E_OVERLAP = 7, RTM3D_OPTIM_E_TOO_MANY = 8, RTM3D_OPTIM_E_LAUNCH = 9 };
typedef struct rtm3d_optim_segment {
    void* p;                               /* parameter (kinds 0, 1: read and written) or buffer (kind 2: read) */
    const void* g;                         /* gradient; kinds 0, 1 */
    void* m;                               /* first moment (exp_avg); kinds 0, 1 */
    void* u;                               /* infinity norm (exp_inf); kinds 0, 1 */
    void* e;                               /* EMA; kinds 0, 2 */
    long long n;                           /* fp32 elements */
    int kind;                              /* RTM3D_OPTIM_UPDATE_EMA / _UPDATE / _EMA */
    int cls;                               /* hyper class, 0 .. 15 (ignored by kind 2) */
} rtm3d_optim_segment;
typedef struct rtm3d_optim_chunk {
    int segment;                           /* row of the segment table */
    int index;                             /* elements index * RTM3D_OPTIM_CHUNK .. of that segment */
} rtm3d_optim_chunk;
typedef struct rtm3d_optim_hyper {         /* the scalars of one step, passed to the launch by value */
    float nclr[RTM3D_OPTIM_MAX_CLASSES];
    float wd[RTM3D_OPTIM_MAX_CLASSES];
    float w, beta2, eps;
    float ema_d, ema_omd;
    int reserved;                          /* 0 */
} rtm3d_optim_hyper;
int rtm3d_optim_table_bytes(int n_segments, const long long* sizes, size_t* segment_bytes, size_t* chunk_bytes, int* n_chunks);
int rtm3d_optim_plan(int n_segments, const rtm3d_optim_segment* segments, rtm3d_optim_segment* segment_table,
                     rtm3d_optim_chunk* chunk_table, int* n_chunks);
/* segments[N]: HOST descriptors holding DEVICE addresses; segment_table[N] and chunk_table[*n_chunks]: HOST memory of the sizes
 * rtm3d_optim_table_bytes names.  Nothing is written when the call refuses. */
int rtm3d_optim_step(void* stream, const rtm3d_optim_segment* d_segment_table, const rtm3d_optim_chunk* d_chunk_table, int n_chunks,
                     const rtm3d_optim_hyper* hyper, const float* d_loss, unsigned* d_skipped);
/* d_segment_table, d_chunk_table: the two tables on the DEVICE; hyper: HOST; d_loss: DEVICE fp32 or NULL; d_skipped: DEVICE uint32. */

/* ---- head backward (rtm3d_amd/head_train.py): from dL/dlogits to the gradients of the detection heads' conv parameters ---------
 * The link between rtm3d_loss_grad and rtm3d_optim_step for the G head branches (models/nets/header.py): per branch a 3x3
 * dilation-6 conv 256 -> 256 + BN + ReLU on the fused map z, (HEADER_NUM_CONV - 1) x [3x3 conv 256 -> 256 + BN + ReLU], and a final
 * 3x3 conv 256 -> K with bias.  The forward's activations (z, h1, h2 ... in the plan's workspace) are the saved activations.
 *
 * DEVIATION: BatchNorm is FROZEN.  Running statistics and the affine pair are constants (FrozenBatchNorm: the function the folded
 * plan computes); the reference trains BN on batch statistics.  Trainable: weight and bias of every head conv.
 *
 * THE RULE.  s = gamma / sqrt(var + eps); Wf = fp16(s w), the folded weight as the forward used it; S a power-of-two grad_scale.
 *   1. go = fp16(S dL/dlogit), gathered from the G fp32 NCHW maps into one NHWC map, 16 channels per head (k >= K: zero).
 *   2. final conv of head g:   dWo[k][c][tap] = (1/S) sum_p go[p][k] h_last[p + tap][c],     dbo[k] = (1/S) sum_p go[p][k]
 *   3. dh_last[p][c] = fp16( [h_last[p][c] > 0] sum_{k, tap} go[p - tap][k] Wo[k][c][tap] )          (Wo = fp16(wo))
 *   4. each 256 -> 256 conv, last to first, with dY the gradient at its output and X its input, dilation d:
 *          dWf[co][ci][tap] = (1/S) sum_p dY[p][co] X[p + d tap][ci],      dbf[co] = (1/S) sum_p dY[p][co]
 *          dX[p][ci] = fp16( [X[p][ci] > 0] sum_{co, tap} dY[p - d tap][co] Wf[co][ci][tap] )   if a conv precedes it or dz is wanted;
 *      z carries no mask, and dz sums over the G branches (one accumulator, branch after branch).
 *   5. dw = s[co] dWf, db = s[co] dbf, in fp32 after the reduction.  The final convs have no BN.
 * tap = (ky - 1, kx - 1), ky-major, as torch's cross-correlation.  Every product is an fp16 x fp16 MFMA product with fp32
 * accumulation; the only fp16 roundings of gradients are the ones written above (dz is stored as fp16 too, still scaled by S).
 * Parameter gradients leave as fp32, unscaled, in torch's (cout, cin, 3, 3) order.  NO FLOAT ATOMICS: the sums over the
 * B H W pixels are cut into slices of whole 32-pixel tiles (rtm3d_head_backward_slices), each slice writes a partial to the
 * workspace, and a second pass adds the partials in slice order - two runs on equal inputs leave equal bytes.  The order of the
 * additions inside a slice is the kernel's (MFMA order) and not part of the rule.  The bias sums use slices of their own: at most
 * 1024 runs of ceil(B H W / 1024) consecutive pixels, added in pixel order inside a run, the runs in index order.  Every produced parameter gradient that is NaN or
 * +-Inf adds 1 to *d_nonfinite (an integer atomic; no host synchronisation).
 *
 * MAPS (rtm3d_hb_map): fp16 NHWC [B][H + 2 P][W + 2 P][C] with a border of P pixels, as rtm3d_tensor_info describes the plan's
 * tensors; branch g's channels are coff + g * gstride .. .  A gradient map needs the border of its reader's taps (go: 1, the
 * gradient at a dilation-d conv's output: d) and that border must be ZERO: the launches write interior pixels only, so a map
 * that was cleared once stays valid.  An activation map needs the border of the conv that read it (z: 6, h: 1).
 *
 * ENTRY POINTS.  All take raw device pointers plus geometry, check on the HOST first and launch nothing when they refuse
 * (RTM3D_HB_E_*, the message in rtm3d_last_error):
 *   E_NULL a NULL argument; E_SHAPE B, H, W outside 1 .. 16384 or B H W >= 2^31; E_GROUPS a branch count other than 1, 2, 4;
 *   E_CHANNELS K outside 1 .. 16, a channel width other than 16 / 256, offsets that are no multiple of 8 or leave the map,
 *   branches of dY that are not adjacent; E_NUM_CONV HEADER_NUM_CONV < 1; E_SCALE a grad_scale that is no power of two;
 *   E_SLICES a slice count outside 1 .. RTM3D_HB_MAX_SLICES (or a refresh job count outside 1 .. RTM3D_HB_MAX_JOBS); E_BORDER a border narrower than the taps; E_ALIGN an address that is
 *   no multiple of 16 (maps, weights, workspace) or 4 (fp32); E_WORKSPACE a workspace that is too small; E_LAUNCH.
 * rtm3d_head_backward_check / _slices / _workspace_bytes are HOST functions and run without a GPU.
 * rtm3d_head_backward_slices: ntiles = ceil(npix / 32); tiles_per_slice = ceil(ntiles / want); n_slices = ceil(ntiles /
 * tiles_per_slice) <= want - every slice but the last holds tiles_per_slice tiles, the last the remainder, none is empty.
 *
 * REFRESH.  After an optimiser step the plan's packed fp16 weights, fp32 biases and the rotated dgrad copies are stale.
 * rtm3d_head_refresh rebuilds them in ONE launch from a table of jobs: packed[i] = fp16(fp32(w[perm[i]] * s[c])) (kind 0) or
 * fp32((b[perm[i]] - mean[c]) * s[c] + beta[c]) (kind 1), the product and the sum in fp64 without contraction - the operations
 * of the host fold, so the bytes are the host packers' bytes.  w / b: one fp32 arena of all parameters; c = scale_of[perm[i]]
 * names a row {s, mean, beta} of the fp64 table bn (a conv without BN: {1, 0, 0}); perm[i] < 0 is a padding element, zero.
 * The caller builds perm ONCE by sending index arrays through the packers and guarantees 0 <= perm[i] < arena size or < 0.
 *
 * OUT OF SCOPE: the backward upstream of dz (dz is the hand-off; "neck fusion backward" below takes it one stage up), training
 * BatchNorm, head_precision = 'mxfp8'.  */
#define RTM3D_HB_MAX_SLICES 256
#define RTM3D_HB_MAX_JOBS 64
enum { RTM3D_HB_E_NULL = 1, RTM3D_HB_E_SHAPE = 2, RTM3D_HB_E_GROUPS = 3, RTM3D_HB_E_CHANNELS = 4, RTM3D_HB_E_NUM_CONV = 5,
       RTM3D_HB_E_SCALE = 6, RTM3D_HB_E_SLICES = 7, RTM3D_HB_E_BORDER = 8, RTM3D_HB_E_ALIGN = 9, RTM3D_HB_E_WORKSPACE = 10,
       RTM3D_HB_E_LAUNCH = 11 };
typedef struct rtm3d_hb_map {
    void* d;                               /* DEVICE address of padded element [0][0][0][0] */
    int C;                                 /* channels of the tensor */
    int P;                                 /* border in pixels */
    int coff;                              /* first channel of branch 0 */
    int gstride;                           /* channels from one branch to the next */
} rtm3d_hb_map;
typedef struct rtm3d_hb_refresh_job {
    void* dst;                             /* DEVICE: fp16 (kind 0) or fp32 (kind 1) array of n elements */
    const void* perm;                      /* DEVICE: n int32 indices into the parameter arena, < 0 for padding */
    long long n;
    int kind;                              /* 0: folded fp16 weights, 1: folded fp32 biases */
    int reserved;                          /* 0 */
} rtm3d_hb_refresh_job;
int rtm3d_head_backward_check(int B, int H, int W, int G, const int* K, int num_conv, float grad_scale);
int rtm3d_head_backward_slices(long long npix, int want, int* n_slices, int* tiles_per_slice);
size_t rtm3d_head_backward_workspace_bytes(int G, int n_slices);      /* 0 for a G or slice count the launches refuse */
/* step 1.  d_dlogit[G]: HOST array of DEVICE fp32 (B, K[g], H, W); go: 16 channels per head, written on the interior. */
int rtm3d_head_go(void* stream, int B, int H, int W, int G, const int* K, const float* const* d_dlogit, float grad_scale,
                  const rtm3d_hb_map* go);
/* steps 2, 4, 5 of one conv layer of all G branches: dY has cout (16: final conv, 256) channels per branch, X 256 with a border
 * >= dil.  d_s[g]: the 256 BN scales or NULL (d_s itself may be NULL); d_dw[g]: (cout_valid[g], 256, 3, 3) fp32 or NULL;
 * d_db[g]: cout_valid[g] fp32 or NULL - a NULL output is skipped and the others are the bits of the full call.  d_ws:
 * rtm3d_head_backward_workspace_bytes(G, n_slices) bytes for the n_slices that `want_slices` gives at B H W pixels. */
int rtm3d_head_wgrad(void* stream, int B, int H, int W, int G, int dil, int cout, const int* cout_valid, const rtm3d_hb_map* dy,
                     const rtm3d_hb_map* x, float grad_scale, const float* const* d_s, float* const* d_dw, float* const* d_db,
                     int want_slices, void* d_ws, size_t ws_bytes, unsigned* d_nonfinite);
/* steps 3, 4: dX of n_out branches, each summing n_sum branches of dY (one of the two counts is 1: n_sum = G gives dz).  dY: kc
 * (16 / 256) channels per branch, zero border >= dil; d_wr: the rotated weights fp16 [branch][tap][ci = 256][kc], element =
 * Wf[co = k][ci][tap]; mask: X (256 channels per output branch) or NULL / d == NULL for none; out: 256 channels per output branch. */
int rtm3d_head_dgrad(void* stream, int B, int H, int W, int n_out, int n_sum, int dil, int kc, const rtm3d_hb_map* dy,
                     const void* d_wr, const rtm3d_hb_map* mask, const rtm3d_hb_map* out);
/* h_jobs: the n_jobs descriptors on the HOST (checked: rtm3d_head_refresh_check, callable without a GPU), d_jobs: the same table on
 * the DEVICE (8-byte aligned); d_bn: fp64 rows {s, mean, beta}. */
int rtm3d_head_refresh_check(int n_jobs, const rtm3d_hb_refresh_job* jobs);
int rtm3d_head_refresh(void* stream, int n_jobs, const rtm3d_hb_refresh_job* h_jobs, const rtm3d_hb_refresh_job* d_jobs,
                       const float* d_arena, const int* d_scale_of, const double* d_bn);

/* ---- neck fusion backward (rtm3d_amd/neck_train.py): from dz to the gradients of the fusion's transposed convs and of kfpn_h* ----
 * The stage upstream of the heads' dz is the fusion half of the neck (models/nets/keypoint_fpn_fusion.py, forward):
 *     z = z0 + sum_i u_i * softmax_{H W}(u_i.detach()),     u_i = fusion_up{i}(kfpn_h{i}),    i = 3, 4, 5
 * where fusion_up{i} is a chain of i - 2 ConvTranspose2d(256, 256, k = 4, s = 2, p = 1, bias = False).  Here the operands are
 * numbered l = 1 .. levels (levels = 3: l = 1 is kfpn_h3's chain of one transposed conv, l = 3 kfpn_h5's chain of three); the
 * input of operand l is (H / 2^l) x (W / 2^l) for the H x W map of z.  The forward's tensors (kfpn_h*, the intermediate up maps,
 * u_l) are the saved activations.
 *
 * THE RULE.  S: the heads' grad_scale.  T: a second power of two, the fusion scale - the softmax weights are about 1 / (H W), so
 * du would underflow fp16 without it.  dz arrives as fp16 NHWC, times S.
 *   1. dz0 = dz.  The SAME tensor: no launch, no copy - the gradient at z0 is the map the head backward wrote.
 *   2. softmax statistics per operand l, image b, channel c:  m = max_p u_l[p],  Z = sum_p exp(u_l[p] - m),  exp in fp32.  The
 *      pixels of an image are cut into at most 32 runs of R = 8 ceil(ceil(H W / 32) / 8) consecutive pixels; a run's (m, Z) is
 *      formed by 8 lanes, lane j taking pixels j, j + 8 .. of the run in that order with a running maximum (Z <- Z exp(m_old -
 *      m_new) + exp(u - m_new)), the 8 lanes are combined in lane order and the runs in index order, each as
 *      Z = sum_k Z_k exp(m_k - max m).  The pass is this code's own: the forward's statistics belong to the plan and are not read.
 *   3. du_l[p][c] = fp16( (T dz[p][c]) * (exp(u_l[p][c] - m) / Z) ), the softmax weight being detached in the reference: this is
 *      the whole derivative.  Written to the interior of a map with a zero border of 1.
 *   4. each transposed conv, last to first, with X (Hi x Wi) its input, dY (2 Hi x 2 Wi, zero border 1) the gradient at its output,
 *      W its (ci, co, ky, kx) weight and Wf = fp16(W) the weight as the forward used it:
 *          dW[ci][co][ky][kx] = 1 / (S T) sum_{b, y, x} X[y][x][ci] dY[2 y + ky - 1][2 x + kx - 1][co]
 *          dX[y][x][ci] = fp16( sum_{ky, kx, co} dY[2 y + ky - 1][2 x + kx - 1][co] Wf[ci][co][ky][kx] )
 *      dX is written on the interior of a map with border 1, which is the next transposed conv's dY; for the first of a chain it is
 *      the FUSION-PATH term of d kfpn_h{i}, times S T (the kfpn_up path of the FPN half adds to it: "neck FPN backward" below).
 *   5. Every product is an fp16 x fp16 MFMA product with fp32 accumulation; the only fp16 roundings of gradients are the ones
 *      written above.  dW leaves as fp32, unscaled, in torch's (cin, cout, 4, 4) order.
 *   6. NO FLOAT ATOMICS.  The wgrad's sum over the B Hi Wi pixels uses the head backward's K-split over slices of whole 32-pixel
 *      tiles (rtm3d_head_backward_slices); partials go to the workspace and are added in slice order, then multiplied by
 *      1 / (S T).  Two runs on equal inputs leave equal bytes.  Every dW element that is NaN or +-Inf adds 1 to *d_nonfinite.
 *
 * MAPS are rtm3d_hb_map with gstride unused: 256 channels from coff on, of a tensor of C channels (a widened tensor: its real C).
 * A gradient map's border must be ZERO; the launches write interiors only, so a map cleared once stays valid.
 *
 * ENTRY POINTS.  Raw device pointers plus geometry; the checks run on the HOST first and nothing is launched when they refuse
 * (RTM3D_NB_E_*, the message in rtm3d_last_error): E_NULL a NULL argument; E_SHAPE B, H, W outside 1 .. 16384 or B H W >= 2^31;
 * E_LEVELS levels (operands) outside 1 .. 3; E_CHANNELS a map that does not hold 256 channels at its offset in steps of 8;
 * E_MULTIPLE a map H or W that is no multiple of 2^levels; E_SCALE a scale that is no power of two (or a product S T outside the
 * fp32 range); E_SLICES a slice count outside 1 .. RTM3D_HB_MAX_SLICES; E_BORDER a border narrower than 1 on a dY / du map;
 * E_ALIGN an address that is no multiple of 16 (4: the counter); E_WORKSPACE a workspace that is too small; E_LAUNCH.
 * rtm3d_neck_backward_check and _workspace_bytes are HOST functions and run without a GPU.
 *
 * The weight refresh after an optimiser step is rtm3d_head_refresh as it is: kind 0, BN row 0 = {1, 0, 0}.
 *
 * OUT OF SCOPE: the FPN half of the neck (kfpn_up*, the composed proj + head 1x1 convs: "neck FPN backward" below) and the backbone
 * backward; graph-replayed plans; head_precision = 'mxfp8'; training BatchNorm.  */
enum { RTM3D_NB_E_NULL = 1, RTM3D_NB_E_SHAPE = 2, RTM3D_NB_E_LEVELS = 3, RTM3D_NB_E_CHANNELS = 4, RTM3D_NB_E_MULTIPLE = 5,
       RTM3D_NB_E_SCALE = 6, RTM3D_NB_E_SLICES = 7, RTM3D_NB_E_BORDER = 8, RTM3D_NB_E_ALIGN = 9, RTM3D_NB_E_WORKSPACE = 10,
       RTM3D_NB_E_LAUNCH = 11 };
int rtm3d_neck_backward_check(int B, int H, int W, int levels, float grad_scale, float fusion_scale);      /* H, W: the map of z */
/* bytes that serve the softmax statistics of `levels` operands at batch B and every wgrad of n_slices slices; 0 for arguments the
 * launches refuse */
size_t rtm3d_neck_backward_workspace_bytes(int B, int levels, int n_slices);
/* steps 2, 3 for n_ops operands (three launches).  dz: H x W, any border; u[n_ops], du[n_ops]: HOST arrays of maps, du with a zero
 * border >= 1. */
int rtm3d_neck_softmax_grad(void* stream, int B, int H, int W, int n_ops, const rtm3d_hb_map* dz, const rtm3d_hb_map* u,
                            const rtm3d_hb_map* du, float fusion_scale, void* d_ws, size_t ws_bytes);
/* step 4, dW of one transposed conv whose input is Hi x Wi.  d_dw: (256, 256, 4, 4) fp32, 16-byte aligned, or NULL (checked, then
 * skipped). */
int rtm3d_neck_deconv_wgrad(void* stream, int B, int Hi, int Wi, const rtm3d_hb_map* x, const rtm3d_hb_map* dy, float grad_scale,
                            float fusion_scale, float* d_dw, int want_slices, void* d_ws, size_t ws_bytes, unsigned* d_nonfinite);
/* step 4, dX.  d_wr: fp16 [tap = 4 ky + kx][ci = 256][co = 256] = Wf.permute(2, 3, 0, 1): no flip and no cin / cout swap, a
 * ConvTranspose2d weight is (ci, co) already. */
int rtm3d_neck_deconv_dgrad(void* stream, int B, int Hi, int Wi, const rtm3d_hb_map* dy, const void* d_wr, const rtm3d_hb_map* dx);

/* ---- neck FPN backward (rtm3d_amd/fpn_train.py): from dz0 to the gradients of the FPN's convs and of the backbone features --------
 * The stage upstream of the fusion is the FPN half of the neck (models/nets/keypoint_fpn_fusion.py, _fpn):
 *     h5 = head5(feat3);   x_{i-1} = proj_i(cat[up_i(h_i), feat_{i-1}]),   h_{i-1} = head_{i-1}(x_{i-1}),   i = 5, 4, 3;   z0 = h2
 * head / proj are 1x1 convs with bias, up_i is ConvTranspose2d(256, 256, k = 4, s = 2, p = 1, bias = False).  Nothing non-linear
 * stands between proj_i and head_{i-1}, and the plan runs the pair as ONE composed 1x1 conv over the concat tensor
 * ncat = [up(256) | feat]:  A = Wh Wp  (256 x Cin),  b = Wh bp + bh.  The backward is taken of that function, on the plan's TRAINING
 * lowering (plan.lower(neck_fold=False)), which keeps ncat*, kfpn_h* and z0 as plain tensors - the saved activations.
 *
 * THE RULE.  S: the heads' grad_scale, T: the fusion scale, U: a third power of two, the fpn scale.  Levels k = 0, 1, 2 name the
 * composed convs from the map of z0 (H x W) upwards: level k works at (H >> k) x (W >> k), X_k = ncat_k (Cin = 320 / 384 / 512 for
 * DLA-34), A_k the composed weight, and its output is z0 (k = 0), kfpn_h3 (k = 1), kfpn_h4 (k = 2).  g_0 = dz, times S.
 *   1. conv1x1 wgrad:   dA[co][ci] = inv sum_p dY[p][co] X[p][ci],    db[co] = inv sum_p dY[p][co]
 *      with dY = g_k and inv the reciprocal of the factor g_k carries (1 / S at k = 0, 1 / (S U) behind it).
 *   2. conv1x1 dgrad:   dX[p][ci] = fp16( mul sum_co dY[p][co] Af[co][ci] ),   Af = fp16(A) as the forward used it,
 *      mul a power of two applied in fp32 before the rounding (U at k = 0, 1 behind it): D_k, Cin channels, times S U.
 *      D_k[:, 256:] is d feat_k; D_k[:, :256] is the gradient at the output of kfpn_up{k+3}.
 *   3. the transposed conv kfpn_up{k+3}: rtm3d_neck_deconv_wgrad (x = kfpn_h{k+3}, dy = D_k[:, :256], grad_scale = S, fusion_scale =
 *      U) and rtm3d_neck_deconv_dgrad into E_k - "neck fusion backward", step 4, unchanged.
 *   4. grad add:   g_{k+1}[p][c] = fp16( fp32(E_k[p][c]) + fp32(F_k[p][c]) r ),   r = U / T,
 *      F_k being the fusion-path term of d kfpn_h{k+3} (times S T): g_{k+1} is the FULL gradient at kfpn_h{k+3}, times S U.
 *   5. after level 2, kfpn_head5: step 1 with X = feat3 (Cin = 512), dY = g_3, and step 2 with mul = 1 into d feat3.
 *   6. THE FACTOR RULE gives the reference's own parameters from the composed gradients, exactly (there is no non-linearity):
 *          dWh = dA Wp^T + db bp^T,   dWp = Wh^T dA,   dbh = db,   dbp = Wh^T db
 *      (head's input is Wp ncat + bp: proj's bias reaches head's weight) - weight-sized products, formed in fp64 by the caller
 *      and stored as fp32.
 *   7. Every product is an fp16 x fp16 MFMA product with fp32 accumulation; the only fp16 roundings of gradients are the ones
 *      written above.  dA, db leave as fp32 in torch's (256, Cin, 1, 1) order.
 *   8. NO FLOAT ATOMICS.  The wgrad's sum over the B H W pixels uses the head backward's K-split over slices of whole 32-pixel
 *      tiles (rtm3d_head_backward_slices); partials go to the workspace and are added in slice order, then multiplied by inv.  The
 *      bias sums use the head backward's rule: at most 1024 runs of ceil(B H W / 1024) consecutive pixels, added in pixel order
 *      inside a run, the runs in index order.  Two runs on equal inputs leave equal bytes.  Every dA / db element that is NaN or
 *      +-Inf adds 1 to *d_nonfinite.
 *
 * MAPS are rtm3d_hb_map with gstride unused: X and dX hold Cin channels from coff on, dY, E, F and g 256, of a tensor of C
 * channels; any border 0 .. 64.  The launches write interiors only, so a gradient map whose border was cleared once stays valid
 * for the transposed conv that reads it.  Cin: a multiple of 64 in 64 .. 1024.
 *
 * ENTRY POINTS.  Raw device pointers plus geometry; the checks run on the HOST first and nothing is launched when they refuse
 * (RTM3D_FB_E_*, the message in rtm3d_last_error): E_NULL a NULL argument; E_SHAPE B, H, W outside 1 .. 16384 or B H W >= 2^31;
 * E_CIN a Cin that is no multiple of 64 in 64 .. 1024; E_CHANNELS a map that does not hold its channels at its offset in steps of
 * 8; E_SCALE an inv / mul / r that is no power of two (or whose reciprocal leaves the fp32 range); E_SLICES a slice count
 * outside 1 .. RTM3D_HB_MAX_SLICES; E_BORDER a border outside 0 .. 64; E_ALIGN an address that is no multiple of 16 (4: db, the
 * counter); E_WORKSPACE a workspace that is too small; E_LAUNCH.
 * rtm3d_fpn_backward_check and _workspace_bytes are HOST functions and run without a GPU.
 *
 * The weight refresh after an optimiser step is rtm3d_head_refresh as it is (kinds 0 and 1, BN row 0 = {1, 0, 0}) over an arena
 * that holds the composed A and b next to the parameters.
 *
 * OUT OF SCOPE: the backbone backward (d feat0 .. d feat3 are the hand-off); graph-replayed plans; head_precision = 'mxfp8';
 * training BatchNorm.  */
enum { RTM3D_FB_E_NULL = 1, RTM3D_FB_E_SHAPE = 2, RTM3D_FB_E_CIN = 3, RTM3D_FB_E_CHANNELS = 4, RTM3D_FB_E_SCALE = 5,
       RTM3D_FB_E_SLICES = 6, RTM3D_FB_E_BORDER = 7, RTM3D_FB_E_ALIGN = 8, RTM3D_FB_E_WORKSPACE = 9, RTM3D_FB_E_LAUNCH = 10 };
int rtm3d_fpn_backward_check(int B, int H, int W, int Cin, float factor);      /* H, W: the conv's own map; factor: an inv, mul or r */
/* bytes that serve one wgrad of n_slices slices at Cin channels (weight partials and the 1024 bias runs); 0 for arguments the
 * launches refuse */
size_t rtm3d_fpn_backward_workspace_bytes(int Cin, int n_slices);
/* step 1.  d_dA: (256, Cin, 1, 1) fp32, 16-byte aligned, or NULL; d_db: 256 fp32 or NULL - a NULL output is skipped and the other
 * is the bits of the full call. */
int rtm3d_fpn_conv1x1_wgrad(void* stream, int B, int H, int W, int Cin, const rtm3d_hb_map* x, const rtm3d_hb_map* dy, float inv,
                            float* d_dA, float* d_db, int want_slices, void* d_ws, size_t ws_bytes, unsigned* d_nonfinite);
/* step 2.  d_wr: fp16 [ci = Cin][co = 256] = Af transposed. */
int rtm3d_fpn_conv1x1_dgrad(void* stream, int B, int H, int W, int Cin, const rtm3d_hb_map* dy, const void* d_wr, float mul,
                            const rtm3d_hb_map* dx);
/* step 4.  g may be E or F itself (each thread reads its own 16 bytes before it writes them). */
int rtm3d_fpn_grad_add(void* stream, int B, int H, int W, const rtm3d_hb_map* e, const rtm3d_hb_map* f, float r, const rtm3d_hb_map* g);

#ifdef __cplusplus
}
#endif
#endif /* RTM3D_HIP_H */
