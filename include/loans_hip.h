/*
 * loans_hip.h -- C ABI of the MI355X (gfx950) kernels behind the LoANs
 * localizer -> STN crop -> assessor training hot path.
 *
 * The reference (Bartzi/loans) has NO FFI of its own: every FLOP of this path
 * is executed inside Chainer 4.1 / CuPy / cuDNN, reached through Chainer's
 * Link / Function interface.  Each entry point below therefore replaces the
 * third-party kernel behind a reference *call site* (cited per function,
 * paths relative to /root/reference).  The Python host in loans_amd/ binds
 * this header with ctypes (loans_amd/_lib.py); INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Contract for every function:
 *   - plain device pointers + explicit sizes; no torch / framework types;
 *   - returns 0 on success, a negative LOANS_E* code for rejected arguments,
 *     or a positive hipError_t from the launch;
 *   - never allocates, frees or synchronises; work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - caller owns every buffer (workspaces included) until the stream passes;
 *   - device = current HIP device of the calling thread; re-entrant and
 *     thread-safe given distinct streams, for any number of devices per
 *     process: the only state the launchers keep is per kernel AND per device
 *     ordinal (the raised dynamic-LDS limit of a kernel, the device's CU
 *     count), held in lock-free tables (csrc/common.h).  The only runtime
 *     calls besides the launch are hipGetDevice (thread-local read) and, once
 *     per (kernel, device), hipFuncSetAttribute / hipDeviceGetAttribute --
 *     none is a stream operation and none blocks, so the first call of an
 *     entry point may sit inside a hipGraph stream capture.
 *
 * Layouts: activations NHWC float32 with C a multiple of 4 (3-channel images
 * are carried as 4 channels, the 4th zero); conv weights "OHWI"
 * [Cout][kh][kw][Cin]; Linear W [out][in].
 */
#ifndef LOANS_HIP_H
#define LOANS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LOANS_OK 0
#define LOANS_EINVAL (-1)   /* bad shape / null pointer / misaligned size */
#define LOANS_ERANGE (-2)   /* size beyond what the kernel's 32-bit indexing supports */

#define LOANS_MAX_TAPS 64
#define LOANS_STATS_REPLICAS 32   /* BN-statistics accumulators are replicated to spread fp64 atomics */

/* epilogue / loader flags of the implicit-GEMM kernels */
#define LOANS_F_RELU_IN   1   /* gather relu(in) instead of in (pre-activation blocks, common/net.py:22,43,44,64,65) */
#define LOANS_F_BIAS      2   /* out += bias[n]                         (sheep/resnet.py:43 conv1) */
#define LOANS_F_STATS     4   /* stats[r][0][n] += sum_m out, stats[r][1][n] += sum_m out^2 (double), r = block % LOANS_STATS_REPLICAS */
#define LOANS_F_MASK      8   /* out = (ref[m][n] > 0) ? out : 0        (ReLU backward folded into dgrad) */
#define LOANS_F_ADDEND   16   /* out += addend[m][n]                    (residual sums; may alias out) */
#define LOANS_F_ADDEND_MASK 32 /* with ADDEND: out += (ref[m][n] > 0) ? addend[m][n] : 0  (identity shortcut through a ReLU) */
#define LOANS_F_DENSE     64   /* dense K rows for packed 3-channel images (conv1 7x7/2, sheep/resnet.py:43): `in` is a zero-padded
                                 [B][inH][inW floats] buffer (loans_prep_images_dense_f32), inW / isx / dx[] count FLOATS,
                                 tap t is the run of Cin consecutive floats at row y*isy + dy[t], float x*isx + dx[t]; w is
                                 [Cout][ntaps][Cin].  No bounds masks: every run must lie inside its row (checked). */

#define LOANS_F_OUT_BF16 128   /* loans_igemm_bf16_f32 only: `out` is a bf16 tensor (fp32 in, bf16 out: the stem conv of the bf16
                                  storage arm); not with MASK / ADDEND */
#define LOANS_F_BNSUMS  512   /* data gradients only (loans_igemm_f32 / loans_igemm_bf16s; no other epilogue flag): the launch's output g is the
                                  gradient that reaches a BatchNormalization whose own ReLU follows it (sheep/resnet.py:137,157).  `ref` is that
                                  BN's INPUT y (same shape as out), `bias` its coefficient table float[4][C] = mean, rstd, scale, shift (C = out
                                  channels) and `stats` fp64 accumulators [LOANS_STATS_REPLICAS][2][C]: the epilogue adds sum_m g m and
                                  sum_m g m (y - mean) with m = (y scale + shift > 0) -- the two sums of that BN's backward, taken from the tile
                                  while it is in registers instead of by a pass over the stored tensor (loans_bn_bwd_reduce_xmask_*); g is
                                  stored unmasked, on bf16 tensors the sums use the ROUNDED g the later passes will read.  Not with split-K /
                                  fine-tail tiles, LOANS_TILE_WS64, class launches. */
#define LOANS_F_AFFINE_IN 1024  /* (round 5) the convolution's input operand is relu(x * scale + shift) rounded to bf16: the BatchNormalization + ReLU in
                                  front of it (bn2 -> conv3 of a bottleneck, sheep/resnet.py:163-216) applied on load, with loans_bn_apply_bf16's
                                  arithmetic bit for bit, so that the activation tensor between them is never written.  Forward LOANS_TILE_PW
                                  launches of loans_igemm_bf16s only (`bias` = float[2][Cin] = scale, shift; with or without LOANS_F_STATS) and
                                  loans_wgrad_bf16s_affine_ws */
#define LOANS_F_GY_BF16  256   /* loans_wgrad_bf16_f32 only: `gy` is a bf16 tensor, x stays fp32 (the stem's weight gradient) */

/*
 * One implicit-GEMM problem:  out[m][n] = sum_{t<ntaps} sum_{c<Cin} in[pix(m,t)][c] * w[n][t][c]
 * m enumerates (b, y, x) over B x gridH x gridW;
 *   output pixel  = (y*osy + oy0, x*osx + ox0)   in an outH x outW x Cout tensor,
 *   gathered pixel = (y*isy + dy[t], x*isx + dx[t]) in an inH x inW x Cin tensor (zero outside).
 * fprop:  isy = stride, dy[t] = r - pad, os = 1.          (F.convolution_2d forward)
 * dgrad:  `in` is the output gradient, one launch per stride-parity class.
 */
typedef struct loans_igemm_desc {
    int32_t B, inH, inW, Cin;
    int32_t outH, outW, Cout;
    int32_t gridH, gridW;
    int32_t osy, osx, oy0, ox0;
    int32_t isy, isx;
    int32_t ntaps;
    int32_t flags;
    int32_t tile;               /* 0 = auto, else LOANS_TILE_* */
    int8_t dy[LOANS_MAX_TAPS];
    int8_t dx[LOANS_MAX_TAPS];
} loans_igemm_desc;

#define LOANS_TILE_128x128 1
#define LOANS_TILE_128x64  2
#define LOANS_TILE_64x64   3
#define LOANS_TILE_256x64  4
#define LOANS_TILE_64x128  5   /* wgrad only: 64 output channels x 128 tap-channel columns */
#define LOANS_TILE_SPLIT   6   /* igemm only: 128x128 tiles over the rows that fill whole machine rounds, 64x64 over the rest (two launches) */
#define LOANS_TILE_256x128 7   /* loans_igemm_bf16s only: one 512-thread block per CU, three LDS stages (chunk c + 2 in flight) */
#define LOANS_TILE_DEEP    32  /* loans_igemm_bf16s, OR-ed onto 128x128 / 128x64 / 64x64: a 4 / 5 / 8-stage LDS ring (3 / 4 / 7 chunks of K in
                                  flight per block) for grids of about one block per CU with a long K (res6 / res7 at 512 px) */
#define LOANS_TILE_256x256PP 43 /* loans_igemm_bf16s only (not LOANS_F_DENSE, no split-K): LOANS_TILE_256x256 with a ping-pong K loop -- waves 0-3 and
                                   4-7 (the two waves of every SIMD) run half a phase apart, one group on the matrix pipe while the other reads
                                   fragments and issues LDS-DMA; operand HALF-tiles re-staged the phase after their last read, counted vmcnt,
                                   raw barriers (csrc/igemm16_pp.h).  Results bit-identical to LOANS_TILE_256x256. */
#define LOANS_TILE_256x256PP16 44 /* LOANS_TILE_256x256PP on v_mfma_f32_16x16x32_bf16 (the shape the chip holds a higher clock on); 32 k values per
                                     MFMA: results agree with the other tiles to the position of rare bf16 roundings, not bit for bit */
#define LOANS_TILE_256x256 9   /* loans_igemm_bf16s only: 512 threads, eight 128 x 64 wave tiles, two LDS stages; 128 FLOP per staged byte */
#define LOANS_TILE_FINETAIL 8  /* loans_igemm_f32, forward geometry (out row = grid pixel), flags BIAS / STATS / RELU_IN / DENSE only:
                                  64x64 tiles; the tiles that share out evenly over the CUs at full K, the remaining ones (fewer than
                                  one per CU) as K-slices behind them in the same launch (raw partial tiles added with atomics to rows
                                  zeroed here, then loans_igemm_finalize_f32 over those rows).  Plain 64x64 when nothing is left over. */
#define LOANS_TILE_STEM    10   /* loans_igemm_f32 with LOANS_F_DENSE, the 7x7 / 2, Cout = 64 forward geometry, flags BIAS / STATS: direct
                                  convolution -- a block stages the input rows of R output rows and the whole weight matrix in LDS
                                  once and feeds the fp32 MFMA from that image (stem.hip); LOANS_EINVAL for frame sizes it does not
                                  cover (R * Wo must be a multiple of 64 for an R in {4, 2, 1} dividing Ho, <= 448 pixels, <= 80 KB).
                                  loans_igemm_bf16_f32 with LOANS_F_OUT_BF16 (the stem of the bf16 arm): the same direct scheme on the
                                  bf16 MFMA in a persistent kernel -- weights rounded once per block into registers, the image staged
                                  as bf16, any frame size whose 2R + 5 rows fit 78 KB next to the output slabs.
                                  loans_wgrad_f32 with LOANS_F_DENSE (flags DENSE only; `splits` ignored): conv1's weight gradient as a
                                  persistent direct kernel -- per output row the 7 input rows and the row's gradient pixels arrive by
                                  LDS-DMA (double-buffered), rows = 64 channels, columns = the 147 real window positions, every wave
                                  keeps the whole 64 x 160 tile in registers over all its units; the three window-padding columns of
                                  dw [64][7][24] are not written.  LOANS_EINVAL when two unit buffers exceed 156 KB.
                                  loans_wgrad_bf16s / _ws with LOANS_F_DENSE (bf16 frame buffer, bf16 gradient; `splits` ignored): the same
                                  scheme on the bf16 MFMA, 16 pixels per step -- both operands read with transposing LDS reads (the
                                  input rows staged as 12-byte cells, one per 16 bytes: a kernel row is one 32-column tile), the next
                                  unit staged through registers; one slab of the workspace per block (loans_wgrad_bf16s_ws_floats
                                  says how many) or, without one, atomics.  LOANS_EINVAL unless Wo % 16 == 0, Wo <= 256 and
                                  inW == 6 (Wo + 3) (even frame widths) */
#define LOANS_TILE_HALO_128    11  /* loans_igemm_bf16s, stride-1 geometries (forward k x k / 1 and its data gradient, k <= 3, Cin % 64 == 0):
                                      a block owns an 8 x 16 pixel tile x 128 output channels and stages the input halo image once
                                      per 64-channel chunk -- a tap is an LDS window shift, not a gather (csrc/halo_bf16.hip) */
#define LOANS_TILE_HALO_128x64 13  /* the same with 64 output channels per block */
#define LOANS_TILE_HALO_128x64S 14 /* 8 x 16 pixels x 64 output channels, Cin = 64, single-buffered image: four blocks per CU */
#define LOANS_TILE_WS64       15  /* 3x3 / 1, Cin = 64, Cout <= 64 (res2 and its data gradient): one persistent 512-thread block per CU, all
                                      nine taps' weights stationary in LDS, halo images double-buffered across 16 x 16 pixel tiles */
#define LOANS_TILE_HALO_256x128 36 /* 16 x 16 pixels x 128 output channels in one 512-thread block per CU (eight 64 x 64 wave tiles): twice the
                                      MFMA work per staged byte of LOANS_TILE_HALO_128 -- the N = 128 layers, too narrow for a 256-column tile */
#define LOANS_TILE_HALO_256x256 42 /* 16 x 16 pixels x 256 output channels in one 512-thread block per CU (eight 128 x 64 wave tiles, the wave layout
                                      of LOANS_TILE_256x256): the 256- and 512-channel 3 x 3 layers (res4 / res5) with their input staged once per
                                      64-channel chunk instead of once per tap -- 329 KB through the L2 -> LDS path per chunk where the implicit GEMM
                                      moves 576 KB; the fp32 staging tile of the epilogue takes two passes */
#define LOANS_TILE_WSW64      37  /* the same layers with the weights stationary and every WAVE on its own unit (2 rows x 16 pixels x 64 channels:
                                      own halo image, own vmcnt, own staging slab): no block barrier after the weights have landed */
#define LOANS_TILE_WGHALO_64   38  /* loans_wgrad_bf16s, stride-1 3 x 3 forward geometries with Cin % 64 == 0, Cout % 64 == 0: a block owns 64 output x 64
                                      input channels x ALL nine taps and walks 8 x 16 pixel tiles; gradient tile and input halo tile staged once per
                                      tile, a tap is a window shift in LDS (csrc/wgrad_halo_bf16.hip).  splits = blocks per channel-tile pair.
                                      loans_wgrad_f32 (flags RELU_IN or none): the same ownership on v_mfma_f32_32x32x2_f32, the reduction
                                      index is the pixel (csrc/wgrad_halo_f32.hip); pixel tiles are 7 x 14, or 7 x 8 where that covers the
                                      frame with fewer padded pixels (ceil(H/7) ceil(W/8) 56 < ceil(H/7) ceil(W/14) 98: the 7 x 7 frame);
                                      fp32 atomics into dw.  LOANS_EINVAL, dw untouched, for any other geometry */
#define LOANS_TILE_WGHALO_128  39  /* the same with 128 output channels per block on eight waves (Cout % 128 == 0) */
#define LOANS_TILE_PW          40  /* loans_igemm_bf16s, 1 x 1 / 1 forward geometries with Cin in {64, 128}, Cout % 64 == 0, Cout <= 512, or Cin = 256,
                                      Cout % 128 == 0, Cout <= 1024; flags STATS or none (ResNet-50's res2 / res3 / res4 bottleneck expansions): a wave owns 32-pixel strips, operands go global -> VGPR
                                      in MFMA fragment layout (never through LDS), output rows leave through a per-wave LDS slab; `w` must be
                                      the weights in FRAGMENT ORDER (loans_pw_pack_bf16).  Outputs bit-identical to the other tiles
                                      (csrc/pw_bf16.hip) */
#define LOANS_TILE_HALO_256x64 12  /* 16 x 16 pixels x 64 output channels, Cin = 64 (one chunk): the res2 convolutions */
#define LOANS_TILE_SPLITK(s) ((s) << 8) /* loans_igemm_f32, OR-ed onto a tile shape, s = 2..255: split-K for small grids (few tiles, long K:
                                  the deep layers at small batch, single-image inference).  Block (tile, i) contracts every s-th
                                  part of K and ADDS its raw partial tile to `out` with fp32 atomics: the caller zero-fills `out`
                                  first (or leaves the addend in it), passes no epilogue flag here, and applies bias / statistics /
                                  mask / addend to the finished sums with loans_igemm_finalize_f32 */
#define LOANS_TILE_DMA    16   /* igemm, fp32 arm, OR-ed onto a tile shape: operand tiles staged by LDS-DMA (buffer_load ... lds)
                                  into XOR-swizzled unpadded LDS rows instead of through registers; same results bit for bit */
#define LOANS_TILE_POSMAJOR 128 /* loans_igemm_f32, OR-ed onto LOANS_TILE_64x64 (| LOANS_TILE_DMA): a row tile holds the SAME grid position of 64
                                  consecutive images instead of 64 consecutive (image, y, x) rows, so the taps that fall outside the frame are
                                  the same for the whole block and its K loop leaves them out (a corner of a 3 x 3 / pad 1 frame runs four
                                  taps of nine).  Cin % 32 == 0, not LOANS_F_DENSE, taps on a grid, B >= 64; an ordinary launch only (no pair,
                                  no classes, no split-K).  The plain tile's sums in the plain tile's order minus the products with a gathered
                                  zero: for finite operands the same output bit for bit up to the sign of an exact zero -- but a non-finite
                                  WEIGHT under a tap that no pixel of the position reads no longer turns the output into NaN.  STATS / BNSUMS
                                  partial sums group other rows (a rounding, as between any two tiles).  LOANS_EINVAL otherwise. */

/* ---- convolution (replaces cuDNN ConvolutionForward / BackwardData / BackwardFilter behind
 *      L.Convolution2D: sheep/resnet.py:43,128-133,151-153 ; common/net.py:15-17,37-39,59-60) ---- */

/* fprop and dgrad. `w` is [Cout][ntaps][Cin] in the launch's tap order. Optional pointers may be NULL
 * when their flag is clear. */
int loans_igemm_f32(const float* in, const float* w, float* out,
                    const float* bias, double* stats, const float* ref, const float* addend,
                    const loans_igemm_desc* d, void* stream);

/* The stride-parity classes of ONE strided data gradient in ONE launch (conv_transpose of a k x k / s convolution is s * s
 * stride-1 correlations over interleaved output pixels -- in the reference a single F.deconvolution_2d inside
 * Convolution2DFunction.backward, reached from every strided convolution of sheep/resnet.py:115-141).  descs[0..n) are the
 * per-class descriptors loans_igemm_f32 would get one launch each; they may differ in gridH / gridW, oy0 / ox0 and the taps
 * (<= LOANS_MAX_CLS_TAPS each) and must agree in everything else; w[c] is class c's [Cout][ntaps_c][Cin] matrix (host array of
 * n device pointers, read before the call returns).  The classes' tiles share one grid -- the longest-K class should come
 * first -- and so one tail.  Flags MASK / ADDEND / ADDEND_MASK / RELU_IN; fp32 arm; descs[0].tile one of 128x128, 128x64,
 * 64x64, 256x64 (| LOANS_TILE_DMA), used for every class. */
#define LOANS_MAX_CLASSES 4
#define LOANS_MAX_CLS_TAPS 16
int loans_igemm_classes_f32(const float* in, const float* const* w, float* out, const float* ref, const float* addend,
                            const loans_igemm_desc* descs, int32_t n, void* stream);

/* Two forward convolutions of the SAME input with the same geometry (kernel, stride, padding, Cin) in ONE launch: BasicA's
 * conv1 and its strided conv shortcut (sheep/resnet.py:128-133), a bottleneck's conv1 and conv4.  `d` describes
 * convolution a (Cout = Cout_a); b differs in weights, Cout_b, output and statistics.  The second one's tiles take the
 * blocks behind the first one's, so the two share one grid and one tail.  Flags STATS / RELU_IN; fp32 arm; tile shapes
 * without LOANS_TILE_SPLIT / LOANS_TILE_SPLITK. */
int loans_igemm_pair_f32(const float* in, const float* w_a, float* out_a, double* stats_a, const float* w_b,
                         float* out_b, double* stats_b, int32_t Cout_b, const loans_igemm_desc* d, void* stream);

/* epilogue of a split-K convolution (LOANS_TILE_SPLITK) over the finished sums, in place on the whole tensor
 * out [rows][C]: (+ bias) (* (ref > 0)) (+ addend [masked by ref > 0]) and the BN statistics of the result; flags as above */
int loans_igemm_finalize_f32(float* out, const float* bias, double* stats, const float* ref, const float* addend,
                             int32_t flags, int64_t rows, int32_t C, void* stream);

/* Same problem with the operands rounded to bf16 (round-to-nearest-even, done while the fp32 tensors are staged
 * into LDS) and contracted on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; every tensor stays fp32 in memory.
 * The "bf16" arm of BASELINE configs 3 / 5 (compute dtype bf16, fp32 accumulate). */
int loans_igemm_bf16_f32(const float* in, const float* w, float* out,
                         const float* bias, double* stats, const float* ref, const float* addend,
                         const loans_igemm_desc* d, void* stream);

/* wgrad: dw[n][t][c] += sum_m gy[opix(m)][n] * x[pix(m,t)][c]   (atomic accumulation into dw).
 * The descriptor is the FORWARD conv's (Cin = x channels, Cout = gy channels; LOANS_F_RELU_IN gathers
 * relu(x)). `splits` = number of m-slices (0 = auto). */
int loans_wgrad_f32(const float* x, const float* gy, float* dw,
                    const loans_igemm_desc* d, int32_t splits, void* stream);

/* wgrad with both operands rounded to bf16 (RNE) and the bf16 MFMA; fp32 accumulation into dw. */
int loans_wgrad_bf16_f32(const float* x, const float* gy, float* dw,
                         const loans_igemm_desc* d, int32_t splits, void* stream);

/* ---- bf16 STORAGE arm (BASELINE configs 3 / 5: "bf16", "bf16 with fp32 grad accumulate").  Activations and
 *      gradients of the localizer's residual stages live in HBM as bf16 NHWC with C % 8 == 0; parameters, their
 *      gradients, BN statistics / coefficients and every accumulation stay fp32.  `void*` = bf16 tensor. ---- */

/* fprop / dgrad on bf16 tensors: in, w ([Cout][ntaps][Cin], see loans_cast_bf16 / loans_repack_dgrad_bf16), out, ref and
 * addend are bf16; bias and stats as in loans_igemm_f32 (statistics are taken from the fp32 accumulators, the output
 * is rounded to bf16 once).  Flags RELU_IN / BIAS / STATS / MASK / ADDEND / ADDEND_MASK; tiles 128x128, 128x64, 64x64,
 * 256x64, 256x128 (0 = auto).  Operand tiles are staged by LDS-DMA, contraction on v_mfma_f32_32x32x16_bf16.
 * LOANS_F_DENSE (here and in loans_wgrad_bf16s): `in` / `x` is the bf16 buffer of loans_prep_images_dense_bf16, inW / isx /
 * dx[] count bf16 ELEMENTS and must be even (the 16-byte K units are then 4-byte aligned), Cin % 8 == 0. */
int loans_igemm_bf16s(const void* in, const void* w, void* out, const float* bias, double* stats,
                      const void* ref, const void* addend, const loans_igemm_desc* d, void* stream);
/* The weights of a 1 x 1 convolution, [Cout][Cin] bf16, in the order LOANS_TILE_PW reads them -- one 1 KiB block per (32 output
 * channels, 16 input channels) MFMA B fragment: packed[((nt * Cin / 16 + ks) * 64 + lane) * 8 + j] =
 * w[nt * 32 + lane % 32][ks * 16 + lane / 32 * 8 + j].  Cout % 32 == 0, Cin % 16 == 0; `packed` holds Cout x Cin bf16. */
int loans_pw_pack_bf16(const void* w, void* packed, int32_t Cout, int32_t Cin, void* stream);
/* The same for every LOANS_TILE_PW layer of a step in ONE launch, from the fp32 master weights (rounded to nearest even): job j packs
 * src [Cout][Cin] fp32 into dst (Cout x Cin bf16, fragment order); first_unit = the sum of Cout x Cin / 8 over the jobs before it,
 * total_units that sum over all jobs.  `jobs_dev` is a table in DEVICE memory, caller-owned, alive until the launch has run. */
typedef struct loans_pw_pack_job {
    const void* src;
    void* dst;
    int32_t Cout, Cin;
    int32_t first_unit, reserved;
} loans_pw_pack_job;
int loans_pw_pack_batch_f32(const loans_pw_pack_job* jobs_dev, int32_t njobs, int32_t total_units, void* stream);
/* Two forward convolutions of the SAME bf16 input with the same geometry AND the same channel count (BasicA's conv1 and its
 * strided conv shortcut, sheep/resnet.py:128-133) as ONE GEMM with 2 x Cout columns: w_ab = [2][Cout][ntaps][Cin] (a's
 * matrix, then b's), out_ab = [2][B][outH][outW][Cout] (two ordinary tensors back to back).  Unlike loans_igemm_pair_f32
 * the two share the staged input tile, not just the grid: at N = 2 x 128 the 256-column tiles apply.  `d` describes
 * convolution a; flags STATS / RELU_IN; Cout % 32 == 0; the implicit-GEMM tiles only. */
int loans_igemm_pair_bf16s(const void* in, const void* w_ab, void* out_ab, double* stats_a, double* stats_b,
                           const loans_igemm_desc* d, void* stream);
/* wgrad with bf16 x and gy, fp32 atomic accumulation into dw ("fp32 grad accumulate"); the pixel-major tiles are staged as
 * they lie and transposed by the fragment reads (ds_read_b64_tr_b16).  Tiles 128x128, 64x64, 64x128, and 256x256 (512 threads, one
 * block per CU) for layers with >= 256 output channels. */
int loans_wgrad_bf16s(const void* x, const void* gy, float* dw, const loans_igemm_desc* d, int32_t splits, void* stream);
/* The same gradient WITHOUT atomics (round 5; replaces the backward-filter of F.convolution_2d at sheep/resnet.py:121-160 like the
 * call above): every block STORES its raw partial tile into slab s = its pixel slice of `ws` ([slabs][Cout][ntaps * Cin] floats, the
 * layout of dw; caller-owned, at least loans_wgrad_bf16s_ws_floats(d, splits) floats, no need to clear it), then
 * loans_fold_slabs_f32 adds the slabs to dw in a FIXED order on the same stream: two runs give bit-identical gradients, and a
 * launch closes with plain 128-byte-row stores plus one streaming pass instead of one fp32 atomic per partial sum (the halo form
 * ends with 18.9 M of them whatever the layer).  dw must not be written by another stream between the two launches. */
int loans_wgrad_bf16s_ws(const void* x, const void* gy, float* dw, const loans_igemm_desc* d, int32_t splits,
                         float* ws, int64_t ws_floats, void* stream);
/* (round 5) the same with LOANS_F_AFFINE_IN in d->flags (1 x 1 / 1 convolutions, the GEMM tiles): `x` is the INPUT of the
 * BatchNormalization in front of the convolution and `affine` its float[2][Cin] = scale, shift; the kernel contracts gy with
 * relu(x * scale + shift) rounded to bf16 -- the tensor loans_bn_apply_bf16 would have written, bit for bit */
int loans_wgrad_bf16s_affine_ws(const void* x, const void* gy, float* dw, const loans_igemm_desc* d, int32_t splits,
                                float* ws, int64_t ws_floats, const float* affine, void* stream);
/* floats of workspace that call takes for (d, splits) -- host arithmetic only, nothing is launched; < 0: a LOANS_E* code */
int64_t loans_wgrad_bf16s_ws_floats(const loans_igemm_desc* d, int32_t splits);
/* dst[i] += ws[0][i] + ws[1][i] + ... + ws[slabs - 1][i] for i < n (n % 4 == 0, 16-byte aligned pointers): every output is summed
 * by ONE thread group in an order that depends on (n, slabs) only -- deterministic, no atomics. */
int loans_fold_slabs_f32(const float* ws, float* dst, int64_t n, int32_t slabs, void* stream);
/* Split-K on bf16 storage for grids that cannot fill the machine (res6 / res7 at 512 px: 2048 - 8192 rows, K = 4608): block
 * (tile, s) contracts every `splits`-th slice of K and ADDS its raw fp32 tile to `partial` [B * outH * outW][Cout] (zeroed by the
 * caller; the descriptor's flags may only carry RELU_IN / DENSE; the implicit-GEMM tiles only); the parity classes of a strided
 * data gradient add into the same buffer.  loans_igemm_finalize_bf16 then writes the bf16 tensor of the finished sums with the
 * epilogue flags BIAS / STATS / MASK / ADDEND / ADDEND_MASK of loans_igemm_bf16s (Cout / 8 must divide 256). */
int loans_igemm_bf16s_splitk(const void* in, const void* w, float* partial, const loans_igemm_desc* d, int32_t splits, void* stream);
int loans_igemm_finalize_bf16(const float* partial, void* out, const float* bias, double* stats, const void* ref,
                              const void* addend, int32_t flags, int64_t rows, int32_t Cout, void* stream);
/* fp32 master weights -> bf16 operand copies: plain cast (n % 4 == 0), and the dgrad re-pack with the cast folded in */
int loans_cast_bf16(const float* src, void* dst, int64_t n, void* stream);
int loans_repack_dgrad_bf16(const float* src, void* dst, int32_t Cout, int32_t Cin, int32_t src_taps,
                            const int32_t* tapsel_host, int32_t ntaps, void* stream);

/* All data-gradient weight re-packs of a step in ONE launch (csrc/weightprep.hip).  `jobs_dev`: a table of `njobs` jobs in DEVICE
 * memory, caller-owned and kept alive while launches that read it are in flight (built once: sources are parameter views of a
 * fixed arena, destinations persistent buffers).  Job i covers the blocks [first_tile, first_tile + tiles_co * tiles_ci * ntaps)
 * with tiles_co = ceil(Cout / 64), tiles_ci = ceil(Cin / 64); first_tile ascending from 0, `total_tiles` = their sum.  Each job
 * is one loans_repack_dgrad_f32 (dst_bf16 = 0) or loans_repack_dgrad_bf16 (dst_bf16 = 1) call with at most
 * LOANS_REPACK_JOB_TAPS selected taps.  Replaces the per-class launches in front of every F.convolution_2d backward-data
 * (sheep/resnet.py:121-160, common/net.py:15-65). */
#define LOANS_REPACK_JOB_TAPS 16
typedef struct loans_repack_job {
    const void* src;            /* fp32 [Cout][src_taps][Cin] */
    void* dst;                  /* [Cin][ntaps][Cout], fp32 or bf16 */
    int32_t Cout, Cin, src_taps, ntaps;
    int32_t tapsel[LOANS_REPACK_JOB_TAPS];
    int32_t first_tile, tiles_co, tiles_ci, dst_bf16;
} loans_repack_job;
int loans_repack_dgrad_batch(const loans_repack_job* jobs_dev, int32_t njobs, int32_t total_tiles, void* stream);

/* dgrad for convolutions whose input has 4 physical channels (the RGB crops, common/net.py:15,17):
 * out[opix(m)][0..3] = sum_t sum_co gy[pix(m,t)][co] * w_ohwi[co][tapsel[t]][0..3]; same descriptor as
 * loans_igemm_f32 (Cin = gy channels, Cout must be 4), flags MASK / ADDEND only. */
int loans_dgrad_c4_f32(const float* gy, const float* w_ohwi, float* out, const float* ref, const float* addend,
                       const loans_igemm_desc* d, const int32_t* tapsel_host, int32_t src_taps, void* stream);

/* same with a bf16 gradient tensor (the assessor's first block in the bf16-storage arm); w, out, ref, addend fp32 */
int loans_dgrad_c4_bf16_f32(const void* gy, const float* w_ohwi, float* out, const float* ref, const float* addend,
                            const loans_igemm_desc* d, const int32_t* tapsel_host, int32_t src_taps, void* stream);

/* The crop gradient as ONE launch (csrc/cropgrad.hip): gx[B][H][W][4] = dgrad_a(gy_a, w_a) + dgrad_b(gy_b, w_b) (+ addend),
 * the two convolutions of DownResBlock1 that read the 4-channel crops (common/net.py:15,17: c0 3x3 / 1, cs 4x4 / 2; the
 * reference's backward runs cuDNN's dgrad twice and adds).  Each gradient tensor [B][outH][outW][C] is read once (taps in
 * the GEMM's N, col2im inside the block); w_* are the FORWARD weights, OHWI [C][k][k][4]; channel 3 of gx is written 0.
 * gy_b / w_b / cb may be NULL (one convolution).  k <= 4, stride <= 2, pad < k, C == 128 (the assessor's width); outH / outW
 * must be the forward output size of an H x W input; each gradient tensor below 2 GiB.  `addend` may alias `out`.
 * `wpack`: caller-owned workspace of LOANS_CROP_WPACK_FLOATS floats (the weights in MFMA fragment order, written by a
 * pre-pass of the same call on the same stream). */
#define LOANS_CROP_WPACK_FLOATS 16384
typedef struct loans_small_conv {
    int32_t k, stride, pad, outH, outW;
} loans_small_conv;
int loans_crop_dgrad_f32(const float* gy_a, const float* w_a, const loans_small_conv* ca, const float* gy_b, const float* w_b,
                         const loans_small_conv* cb, float* out, const float* addend, float* wpack, int32_t B, int32_t H,
                         int32_t W, int32_t C, void* stream);
/* same with bf16 gradient tensors (bf16-storage arm); weights, addend and gx fp32.  The contraction runs on bf16 MFMAs with fp32
 * accumulation: the call's packing pre-pass rounds the weights to bf16 (RNE) into `wpack` (round 6; on fp32 MFMAs the kernel was
 * bound by the matrix pipe: 56 GFLOP at B = 256). */
int loans_crop_dgrad_bf16_f32(const void* gy_a, const float* w_a, const loans_small_conv* ca, const void* gy_b, const float* w_b,
                              const loans_small_conv* cb, float* out, const float* addend, float* wpack, int32_t B, int32_t H,
                              int32_t W, int32_t C, void* stream);

/* weight repack for dgrad: dst[ci][t][co] = src[co][tapsel[t]][ci]  (src is OHWI with `src_taps` taps) */
int loans_repack_dgrad_f32(const float* src, float* dst, int32_t Cout, int32_t Cin, int32_t src_taps,
                           const int32_t* tapsel_host, int32_t ntaps, void* stream);

/* ---- preprocessing (replaces the per-image PIL round trip of resnet.prepare,
 *      sheep/sheep_localizer.py:45,72-82): NCHW RGB [0,1] -> trunc_u8(x*255) -> BGR - mean -> NHWC4 ---- */
int loans_prep_images_f32(const float* images_nchw, float* out_nhwc4, int32_t B, int32_t H, int32_t W, void* stream);
/* same arithmetic, written as packed 3-channel rows into a zero-padded [B][Hp][Wp][3] buffer with the image at
 * (pad, pad): the LOANS_F_DENSE input of conv1.  Every element of the buffer is written. */
int loans_prep_images_dense_f32(const float* images_nchw, float* out_padded, int32_t B, int32_t H, int32_t W,
                                int32_t pad, int32_t Hp, int32_t Wp, void* stream);
/* the same buffer in bf16 (rounded to nearest even, exactly what the bf16 arm's operand staging does to the fp32 one):
 * the LOANS_F_DENSE input of loans_igemm_bf16s / loans_wgrad_bf16s (bf16 storage arm, BASELINE configs 3 / 5) */
int loans_prep_images_dense_bf16(const float* images_nchw, void* out_padded, int32_t B, int32_t H, int32_t W,
                                 int32_t pad, int32_t Hp, int32_t Wp, void* stream);
/* NCHW (C=3) -> NHWC4 without arithmetic (the assessor's `real` batch, sheep_updater.py:32-35) */
int loans_nchw3_to_nhwc4_f32(const float* in, float* out, int32_t B, int32_t H, int32_t W, void* stream);

/* ---- batch normalisation (replaces cuDNN BatchNormalizationForwardTraining/Backward behind
 *      L.BatchNormalization, sheep/resnet.py:44,129-134,152-154; eps 2e-5, decay 0.9) ---- */

/* stats (double [LOANS_STATS_REPLICAS][2][C]: sum, sum of squares over `count` rows) -> mean, rstd, scale=gamma*rstd,
 * shift=beta-mean*scale; updates running stats in place (unbiased var, + eps if eps_in_running_var). */
int loans_bn_finalize_f32(const double* stats, int32_t C, int64_t count, float eps, float decay,
                          const float* gamma, const float* beta, float* running_mean, float* running_var,
                          int32_t eps_in_running_var,
                          float* mean, float* rstd, float* scale, float* shift, void* stream);
/* test-mode coefficients from the running statistics */
int loans_bn_eval_coeffs_f32(int32_t C, float eps, const float* gamma, const float* beta,
                             const float* running_mean, const float* running_var,
                             float* mean, float* rstd, float* scale, float* shift, void* stream);

/* y = act(x*scale+shift [+ r | + x2*scale2+shift2]);  mode 0: no second term, 1: + r, 2: + bn(x2). relu!=0 -> ReLU */
int loans_bn_apply_f32(const float* x, const float* scale, const float* shift,
                       const float* x2, const float* scale2, const float* shift2,
                       float* y, int64_t rows, int32_t C, int32_t mode, int32_t relu, void* stream);

/* stem: y = max_pool_3x3_s2_cover_all(relu(x*scale+shift)); idx = argmax position 0..8 (first maximum)
 * (sheep/resnet.py:72-73). */
int loans_bn_relu_maxpool_f32(const float* x, const float* scale, const float* shift, float* y, uint8_t* idx,
                              int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);
/* (round 5) the same, and xsel[pooled element] = the RAW x at its argmax ([B][OH][OW][C], the type of x): the sums of the stem's
 * BN backward are then loans_bn_bwd_reduce_rep_* (mask kind 2) over (gy, xsel) -- two contiguous pooled-size tensors -- instead of
 * loans_pool_bn_bwd_reduce_*'s gather out of the four times larger x through idx (BackwardData of F.max_pooling_2d +
 * F.batch_normalization, sheep/resnet.py:72-73).  LOANS_EINVAL for channel counts the 16-byte-unit kernel does not tile. */
int loans_bn_relu_maxpool_sel_f32(const float* x, const float* scale, const float* shift, float* y, uint8_t* idx, float* xsel,
                                  int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);
int loans_bn_relu_maxpool_sel_bf16(const void* x, const float* scale, const float* shift, void* y, uint8_t* idx, void* xsel,
                                   int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);
/* gx = (sum over windows whose argmax is this pixel of gy) * (x*scale+shift > 0) */
int loans_maxpool_relu_bwd_f32(const float* gy, const uint8_t* idx, const float* x, const float* scale,
                               const float* shift, float* gx,
                               int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);

/* the same three passes on bf16 tensors (x, x2, y / gy, gx, idx as above; coefficients fp32) */
int loans_bn_apply_bf16(const void* x, const float* scale, const float* shift,
                        const void* x2, const float* scale2, const float* shift2,
                        void* y, int64_t rows, int32_t C, int32_t mode, int32_t relu, void* stream);
int loans_bn_relu_maxpool_bf16(const void* x, const float* scale, const float* shift, void* y, uint8_t* idx,
                               int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);
int loans_maxpool_relu_bwd_bf16(const void* gy, const uint8_t* idx, const void* x, const float* scale,
                                const float* shift, void* gx,
                                int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);

/* backward reductions: sums[0][c] += sum g, sums[1][c] += sum g*xhat  with g = gy*(mask>0) (mask may be
 * NULL), xhat = (x-mean)*rstd. If x2 != NULL also sums[2], sums[3] for (x2, mean2, rstd2).
 * C % 4 == 0 and C / 4 <= 256 or a multiple of 256 (LOANS_EINVAL otherwise); the same holds for loans_colsum_*. */
int loans_bn_bwd_reduce_f32(const float* gy, const float* mask, const float* x, const float* mean,
                            const float* rstd, const float* x2, const float* mean2, const float* rstd2,
                            double* sums, int64_t rows, int32_t C, void* stream);
/* from the sums: ggamma += , gbeta += , and the coefficients of gx = k1*g + k2*x + k3 */
int loans_bn_bwd_coeffs_f32(const double* sums, int32_t C, int64_t count, const float* gamma,
                            const float* mean, const float* rstd, float* ggamma, float* gbeta,
                            float* k1, float* k2, float* k3, void* stream);
/* BN-backward reduction into REPLICATED accumulators (round 3; replaces loans_bn_bwd_reduce_* / _bits_* / _xmask_* where the
 * channel count allows it: C / V a divisor of 256, V = 4 fp32 / 8 bf16 channels = one 16-byte unit): one entry per storage type,
 * mask_kind 0 = none, 1 = g (mask > 0), 2 = g (x scale + shift > 0), 3 = sign bits.  `sums` fp64 [replicas][2][C], dual (x2 given)
 * [replicas][4][C] = [sum g | sum g xhat | sum g | sum g xhat2], zeroed by the caller; blocks add into replica block % replicas
 * (thousands of blocks on 2 C addresses cost more than the pass).  F.batch_normalization's backward, sheep/resnet.py:129-134. */
int loans_bn_bwd_reduce_rep_f32(const float* gy, const void* mask, int32_t mask_kind, const float* x, const float* mean,
                                const float* rstd, const float* x2, const float* mean2, const float* rstd2, const float* scale,
                                const float* shift, double* sums, int32_t replicas, int64_t rows, int32_t C, void* stream);
int loans_bn_bwd_reduce_rep_bf16(const void* gy, const void* mask, int32_t mask_kind, const void* x, const float* mean,
                                 const float* rstd, const void* x2, const float* mean2, const float* rstd2, const float* scale,
                                 const float* shift, double* sums, int32_t replicas, int64_t rows, int32_t C, void* stream);
/* the stem tail's reduction (loans_pool_bn_bwd_reduce_*) into replicated accumulators [replicas][2][C] (round 3) */
int loans_pool_bn_bwd_reduce_rep_f32(const float* gy, const uint8_t* idx, const float* x, const float* scale, const float* shift,
                                     const float* mean, const float* rstd, double* sums, int32_t replicas, int32_t B, int32_t H,
                                     int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);
int loans_pool_bn_bwd_reduce_rep_bf16(const void* gy, const uint8_t* idx, const void* x, const float* scale, const float* shift,
                                      const float* mean, const float* rstd, double* sums, int32_t replicas, int32_t B, int32_t H,
                                      int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);
/* loans_pool_bn_bwd_apply_* with the bias-gradient sums (gxsum) going into `replicas` accumulators gxsum_rep[replicas][C], zeroed by
 * the caller and folded into the bias gradient by loans_fold_replicas_f32 (dst[c] += sum_r src[r][c]): every block closes with C float
 * atomics, and on ONE set of addresses they made the pass slower the more blocks it had.  C / 4 must divide 256.  (round 3) */
int loans_pool_bn_bwd_apply_rep_f32(const float* gy, const uint8_t* idx, const float* x, const float* scale, const float* shift,
                                    const float* k1, const float* k2, const float* k3, float* gx, float* gxsum_rep, int32_t replicas,
                                    int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);
int loans_pool_bn_bwd_apply_rep_bf16(const void* gy, const uint8_t* idx, const void* x, const float* scale, const float* shift,
                                     const float* k1, const float* k2, const float* k3, void* gx, float* gxsum_rep, int32_t replicas,
                                     int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);
int loans_fold_replicas_f32(const float* src, float* dst, int32_t replicas, int32_t C, void* stream);
/* loans_bn_bwd_coeffs_f32 from `replicas` (<= 32) accumulators `rep_stride` doubles apart, each [sum g | second sum][C]; centred = 1:
 * the second sum is sum g (y - mean) as a data gradient's epilogue took it (LOANS_F_BNSUMS), centred = 0: it is sum g xhat */
int loans_bn_bwd_coeffs_rep_f32(const double* sums, int32_t replicas, int32_t rep_stride, int32_t centred, int32_t C, int64_t count,
                                const float* gamma, const float* mean, const float* rstd, float* ggamma, float* gbeta, float* k1,
                                float* k2, float* k3, void* stream);
/* gx = k1*g + k2*x + k3, g = gy*(mask>0); optional second output for (x2, k1b, k2b, k3b) */
int loans_bn_bwd_apply_f32(const float* gy, const float* mask, const float* x,
                           const float* k1, const float* k2, const float* k3, float* gx,
                           const float* x2, const float* k1b, const float* k2b, const float* k3b, float* gx2,
                           int64_t rows, int32_t C, void* stream);

/* ReLU mask as sign bits: loans_bn_apply_bits_* is loans_bn_apply_* that also writes signbits[rows * C / 4], one byte per four
 * channels, bit e = (y[4i + e] > 0); loans_bn_bwd_{reduce,apply}_bits_* are the backward passes taking those bits where the
 * plain ones take the mask tensor -- the final BN of a residual unit, whose mask is the unit's output relu(bn(x) + shortcut)
 * (sheep/resnet.py:141,160): 1/16 (fp32) or 1/8 (bf16) of the activation's bytes in both passes. */
int loans_bn_apply_bits_f32(const float* x, const float* scale, const float* shift,
                            const float* x2, const float* scale2, const float* shift2,
                            float* y, uint8_t* signbits, int64_t rows, int32_t C, int32_t mode, int32_t relu, void* stream);
int loans_bn_apply_bits_bf16(const void* x, const float* scale, const float* shift,
                             const void* x2, const float* scale2, const float* shift2,
                             void* y, uint8_t* signbits, int64_t rows, int32_t C, int32_t mode, int32_t relu, void* stream);
int loans_bn_bwd_reduce_bits_f32(const float* gy, const uint8_t* signbits, const float* x, const float* mean,
                                 const float* rstd, const float* x2, const float* mean2, const float* rstd2,
                                 double* sums, int64_t rows, int32_t C, void* stream);
int loans_bn_bwd_reduce_bits_bf16(const void* gy, const uint8_t* signbits, const void* x, const float* mean,
                                  const float* rstd, const void* x2, const float* mean2, const float* rstd2,
                                  double* sums, int64_t rows, int32_t C, void* stream);
int loans_bn_bwd_apply_bits_f32(const float* gy, const uint8_t* signbits, const float* x,
                                const float* k1, const float* k2, const float* k3, float* gx,
                                const float* x2, const float* k1b, const float* k2b, const float* k3b, float* gx2,
                                int64_t rows, int32_t C, void* stream);
int loans_bn_bwd_apply_bits_bf16(const void* gy, const uint8_t* signbits, const void* x,
                                 const float* k1, const float* k2, const float* k3, void* gx,
                                 const void* x2, const float* k1b, const float* k2b, const float* k3b, void* gx2,
                                 int64_t rows, int32_t C, void* stream);

/* The same two passes for a BN whose own ReLU supplies the mask (relu(bn(x)), the inner BNs of a residual unit,
 * sheep/resnet.py:137,157): g = gy * (x*scale+shift > 0) with the pre-activation recomputed from x -- no mask tensor. */
int loans_bn_bwd_reduce_xmask_f32(const float* gy, const float* x, const float* scale, const float* shift,
                                  const float* mean, const float* rstd, double* sums, int64_t rows, int32_t C, void* stream);
int loans_bn_bwd_apply_xmask_f32(const float* gy, const float* x, const float* scale, const float* shift,
                                 const float* k1, const float* k2, const float* k3, float* gx, int64_t rows, int32_t C,
                                 void* stream);
int loans_bn_bwd_reduce_xmask_bf16(const void* gy, const void* x, const float* scale, const float* shift,
                                   const float* mean, const float* rstd, double* sums, int64_t rows, int32_t C, void* stream);
int loans_bn_bwd_apply_xmask_bf16(const void* gy, const void* x, const float* scale, const float* shift,
                                  const float* k1, const float* k2, const float* k3, void* gx, int64_t rows, int32_t C,
                                  void* stream);

/* The stem's tail fused (sheep/resnet.py:72-73 backwards: max_pooling_2d -> relu -> bn1): with
 * g = (sum over windows whose argmax is this pixel of gy) * (x*scale+shift > 0) never written to memory,
 * reduce: sums[0][c] += sum g, sums[1][c] += sum g*xhat (one gather of x per pooled element);
 * apply:  gx = k1*g + k2*x + k3 (k from loans_bn_bwd_coeffs_f32); gxsum (may be NULL; needs C/4 to divide 256):
 *         gxsum[c] += sum of gx over pixels = the bias gradient of the convolution in front of the BN.
 * gy, idx: [B][OH][OW][C]; x, gx: [B][H][W][C]. */
int loans_pool_bn_bwd_reduce_f32(const float* gy, const uint8_t* idx, const float* x, const float* scale,
                                 const float* shift, const float* mean, const float* rstd, double* sums,
                                 int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);
int loans_pool_bn_bwd_apply_f32(const float* gy, const uint8_t* idx, const float* x, const float* scale,
                                const float* shift, const float* k1, const float* k2, const float* k3, float* gx,
                                float* gxsum, int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);
int loans_pool_bn_bwd_reduce_bf16(const void* gy, const uint8_t* idx, const void* x, const float* scale,
                                  const float* shift, const float* mean, const float* rstd, double* sums,
                                  int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);
int loans_pool_bn_bwd_apply_bf16(const void* gy, const uint8_t* idx, const void* x, const float* scale,
                                 const float* shift, const float* k1, const float* k2, const float* k3, void* gx,
                                 float* gxsum, int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void* stream);

/* bf16 tensors (gy, mask, x, x2, gx, gx2), fp32 sums and coefficients */
int loans_bn_bwd_reduce_bf16(const void* gy, const void* mask, const void* x, const float* mean,
                             const float* rstd, const void* x2, const float* mean2, const float* rstd2,
                             double* sums, int64_t rows, int32_t C, void* stream);
int loans_bn_bwd_apply_bf16(const void* gy, const void* mask, const void* x,
                            const float* k1, const float* k2, const float* k3, void* gx,
                            const void* x2, const float* k1b, const float* k2b, const float* k3b, void* gx2,
                            int64_t rows, int32_t C, void* stream);

/* ---- small dense ops ---- */
/* out[c] += sum_rows x[row][c]   (conv bias gradient) */
int loans_colsum_f32(const float* x, float* out, int64_t rows, int32_t C, void* stream);
int loans_colsum_bf16(const void* x, float* out, int64_t rows, int32_t C, void* stream);
/* _global_average_pooling_2d (sheep_localizer.py:58): x [B][HW][C] -> y [B][C] ; backward broadcast */
int loans_gap_fwd_f32(const float* x, float* y, int32_t B, int32_t HW, int32_t C, void* stream);
int loans_gap_bwd_f32(const float* gy, float* gx, int32_t B, int32_t HW, int32_t C, void* stream);
/* the boundary of the bf16 region: pooled features leave it as fp32, their gradient enters it as bf16 */
int loans_gap_fwd_bf16_f32(const void* x, float* y, int32_t B, int32_t HW, int32_t C, void* stream);
int loans_gap_bwd_f32_bf16(const float* gy, void* gx, int32_t B, int32_t HW, int32_t C, void* stream);
/* L.Linear (sheep_localizer.py:60 ; common/net.py:81,90). act_in: 1 = relu(x) on load; act_out: 1 = sigmoid */
int loans_linear_fwd_f32(const float* x, const float* W, const float* b, float* y,
                         int32_t B, int32_t K, int32_t N, int32_t act_in, int32_t act_out, void* stream);
/* gz = gy (act_out 0) or gy*y*(1-y) (act_out 1). gx[b][k] = sum_n gz W (times x>0 if act_in);
 * gW[n][k] += sum_b gz relu?(x); gb[n] += sum_b gz. gx / gW / gb may be NULL. */
int loans_linear_bwd_f32(const float* x, const float* W, const float* y, const float* gy,
                         float* gx, float* gW, float* gb,
                         int32_t B, int32_t K, int32_t N, int32_t act_in, int32_t act_out, void* stream);
/* the same layer with x (and gx) as bf16 tensors; W, y, gy, gW, gb fp32 */
int loans_linear_fwd_bf16(const void* x, const float* W, const float* b, float* y,
                          int32_t B, int32_t K, int32_t N, int32_t act_in, int32_t act_out, void* stream);
int loans_linear_bwd_bf16(const void* x, const float* W, const float* y, const float* gy,
                          void* gx, float* gW, float* gb,
                          int32_t B, int32_t K, int32_t N, int32_t act_in, int32_t act_out, void* stream);
/* L.Linear with 9 <= N <= 65536 outputs (the ImageNet heads: fc 512 -> 1000, fc6 2048 -> 1000), fp32 on the matrix cores.
 * y[B][N] = x[B][K] W[N][K]^T + b (b may be NULL).  Limits: B in [1, 65536], K in [4, 65536] with K % 4 == 0, N in [9, 65536],
 * every tensor under 2^31 elements; anything else is refused (LOANS_EINVAL / LOANS_ERANGE).  No atomics: two launches on the
 * same inputs give the same bits. */
int loans_linear_wide_fwd_f32(const float* x, const float* W, const float* b, float* y,
                              int32_t B, int32_t K, int32_t N, void* stream);
/* gx[b][k] = sum_n gy W (written); gW[n][k] += sum_b gy x; gb[n] += sum_b gy.  Each of gx / gW / gb may be NULL (not all);
 * W is needed for gx, x for gW. */
int loans_linear_wide_bwd_f32(const float* x, const float* W, const float* gy, float* gx, float* gW, float* gb,
                              int32_t B, int32_t K, int32_t N, void* stream);
/* F.softmax_cross_entropy(z, t, normalize=True, ignore_label=-1) and F.accuracy(z, t) in one pass over z [B][N] (N <= 8192,
 * B <= 65536).  t: int32 labels; a label outside [0, N) -- -1 or anything else -- marks an ignored row (loss 0, gz row 0).
 * count = max(#rows not ignored, 1).  gz[B][N] = (softmax(z) - onehot(t)) / count;  row_loss[B], row_hit[B]: per-row loss and
 * (argmax == t, first index wins a tie);  out[0] = sum(row_loss) / count, out[1] = sum(row_hit) / B, both summed in a fixed order. */
int loans_softmax_xent_fwd_f32(const float* z, const int32_t* t, float* gz, float* row_loss, float* row_hit,
                               float* out, int32_t B, int32_t N, void* stream);
/* The same with a label-smoothed target and a top-k hit: q = (1 - eps) onehot(t) + eps / N (uniform over all N classes, the
 * convention of torch's label_smoothing), row_loss = lse - (1 - eps) z_t - eps mean(z), gz = (softmax(z) - q) / count.  count and
 * ignored rows as above (an ignored row: loss 0, gz row 0, row_hit 0, row_hitk 0).  row_hitk[b] = 1 iff
 * #{ j : z_j > z_t or (z_j == z_t and j < t) } < k -- for k = 1 that is row_hit; k > N: every valid row hits.
 * out[0] = sum(row_loss) / count, out[1] = sum(row_hit) / B, out[2] = sum(row_hitk) / B, summed in a fixed order.  eps == 0
 * gives the bits of loans_softmax_xent_fwd_f32 in out[0], out[1], gz, row_loss and row_hit.  Limits as above, 0 <= eps < 1, k >= 1. */
int loans_softmax_xent_ls_fwd_f32(const float* z, const int32_t* t, float* gz, float* row_loss, float* row_hit,
                                  float* row_hitk, float* out /* [3] */, int32_t B, int32_t N, double eps, int32_t k,
                                  void* stream);
/* The same against a TWO-LABEL target (a mixup / CutMix batch): with w = lam onehot(ta) + oml onehot(tb) (ta == tb: lam + oml on
 * that class), q = (1 - eps) w + eps / N, row_loss = lse - (1 - eps) (lam z_ta + oml z_tb) - eps mean(z), gz = (softmax(z) - q) / count.
 * The weights are taken as they are (the caller makes them sum to one).  A row counts when BOTH labels lie in [0, N); any other
 * row has loss 0, gz 0 and no hit.  row_hit / row_hitk are taken against the dominant label, ta if lam >= oml, else tb, by the
 * rules above.  out as above.  The weights (1, 0) run loans_softmax_xent_ls_fwd_f32 on (z, ta), the weights (0, 1) on (z, tb):
 * every output carries that entry's bits and the label of weight zero is not read (it does not decide whether a row counts).
 * Limits as above; LOANS_EINVAL also for a non-finite weight. */
int loans_softmax_xent_mix_fwd_f32(const float* z, const int32_t* ta, const int32_t* tb, float lam, float oml,
                                   float* gz, float* row_loss, float* row_hit, float* row_hitk, float* out /* [3] */,
                                   int32_t B, int32_t N, double eps, int32_t k, void* stream);
/* Per-class sigmoid binary cross-entropy against the same two-label target q = (1 - eps) w + eps / N, made 0 / 1 by the strict
 * comparison q > thresh where thresh >= 0 (a negative thresh: no threshold).  With e = exp(-|z|):
 * row_loss = sum_i max(z_i, 0) - z_i q_i + log1p(e_i) (finite for every finite z), gz = (sigmoid(z) - q) / denom with
 * denom = count * N (the mean over classes, torch's binary_cross_entropy_with_logits) or count (sum_classes != 0: the sum over
 * classes, the mean over rows), rounded to fp32 once.  out[0] = sum(row_loss) / denom; rows that count, row_hit, row_hitk,
 * out[1] and out[2] as for loans_softmax_xent_mix_fwd_f32.  The weights (1, 0) / (0, 1) are the one-label loss on ta / on tb: the
 * label of weight zero is not read and does not decide whether a row counts; tb == NULL is one label with the weights (1, 0).
 * No atomics: two runs give the same bits.  Limits as above; LOANS_EINVAL also for a non-finite weight, thresh >= 1 or NaN. */
int loans_sigmoid_bce_fwd_f32(const float* z, const int32_t* ta, const int32_t* tb, float lam, float oml,
                              float* gz, float* row_loss, float* row_hit, float* row_hitk, float* out /* [3] */,
                              int32_t B, int32_t N, double eps, int32_t k, float thresh, int32_t sum_classes, void* stream);
/* Knowledge distillation: the two-label loss above mixed with the KL divergence from a frozen teacher's logits zt [B][N] at the
 * temperature T (Hinton's convention; torch's kl_div(log_softmax(z / T), softmax(zt / T), reduction='batchmean') * T * T).  With
 * invT = fl((float)(1 / T)), the rounded products zs = z invT, zts = zt invT, p = softmax(zts), s = softmax(zs), y = softmax(z):
 *   hard = lse(z) - sum_i q_i z_i (the mix entry's row loss),  kl = sum_i p_i ((zts_i - lse(zts)) - (zs_i - lse(zs))),
 *   row_kl = T^2 kl,  row_loss = (1 - alpha) hard + alpha row_kl,  gz = ((1 - alpha)(y - q) + alpha T (s - p)) / count.
 * kl is formed from shifted logits, never from log(p): finite for every finite pair of rows.  Rows that count, row_hit, row_hitk
 * (on z) and out[0..2] as for loans_softmax_xent_mix_fwd_f32; row_thit[b] = (argmax zt_b == the dominant label), first index on a
 * tie; out[3] = sum(row_kl) / count, out[4] = sum(row_thit) / B.  A row that does not count has zeros everywhere.  The weights
 * (1, 0) / (0, 1) are the one-label loss on ta / on tb: the label of weight zero is not read and does not decide whether a row
 * counts.  alpha == 0 runs loans_softmax_xent_mix_fwd_f32 itself -- its bits in gz, row_loss, row_hit, row_hitk, out[0..2] -- does
 * not read zt (which may be NULL) and writes zeros to row_kl, row_thit, out[3], out[4].  No atomics: two runs give the same bits.
 * Limits as above; LOANS_EINVAL also for a non-finite weight, alpha outside [0, 1], T outside [2^-6, 2^6] (a NaN too), and a
 * NULL zt at alpha > 0. */
int loans_softmax_distill_fwd_f32(const float* z, const float* zt, const int32_t* ta, const int32_t* tb, float lam, float oml,
                                  float* gz, float* row_loss, float* row_hit, float* row_hitk, float* row_kl, float* row_thit,
                                  float* out /* [5] */, int32_t B, int32_t N, double eps, int32_t k, double alpha, double T,
                                  void* stream);
/* Evaluation: the plain loss (eps = 0), the top-1 and the top-k hit of every row as defined above, summed into running totals;
 * no gradient is written.  rows: 3 * B floats of scratch (row loss, hit, top-k hit).  acc[5], doubles, read-modify-write:
 * acc[0] += sum of row losses, acc[1] += top-1 hits, acc[2] += top-k hits, acc[3] += rows not ignored, acc[4] += B.  The five sums
 * of the batch are formed in double in a fixed order and added by one thread: no atomics, two runs give the same bits.
 * Limits as above, k >= 1. */
int loans_softmax_xent_eval_f32(const float* z, const int32_t* t, float* rows /* scratch, 3*B floats */,
                                double* acc /* 5 doubles, read-modify-write */,
                                int32_t B, int32_t N, int32_t k, void* stream);
/* y[i] = x[i] * s[0], s on the device (the loss's upstream gradient times gz) */
int loans_scale_by_scalar_f32(const float* x, const float* s, float* y, int64_t n, void* stream);
/* y = x * mask (elementwise, n floats) -- RotationDropout forward/backward (functions/rotation_droput.py:26-48) */
int loans_mul_f32(const float* x, const float* mask, float* y, int64_t n, void* stream);
/* y = a*x + b*y */
int loans_axpby_f32(float a, const float* x, float b, float* y, int64_t n, void* stream);

/* ---- spatial transformer (replaces cuDNN SpatialTf*; sheep_localizer.py:62-63) ---- */
/* grid [B][2][th][tw] (channel 0 = x) from theta [B][2][3] */
int loans_st_grid_fwd_f32(const float* theta, float* grid, int32_t B, int32_t th, int32_t tw, void* stream);
int loans_st_grid_bwd_f32(const float* ggrid, float* gtheta, int32_t B, int32_t th, int32_t tw, void* stream);
/* bilinear, align-corners, one-pixel zero border. images NCHW (C=3) ; rois NHWC4 [B][th][tw][4] */
int loans_st_sampler_fwd_f32(const float* images_nchw, const float* grid, float* rois_nhwc4,
                             int32_t B, int32_t H, int32_t W, int32_t th, int32_t tw, void* stream);
/* ggrid [B][2][th][tw] (+= if accumulate) from grois NHWC4 */
int loans_st_sampler_bwd_grid_f32(const float* images_nchw, const float* grid, const float* grois_nhwc4,
                                  float* ggrid, int32_t accumulate,
                                  int32_t B, int32_t H, int32_t W, int32_t th, int32_t tw, void* stream);

/* ---- losses (sheep_updater.py:42-46,60 ; common/utils.py:142-178,301-316) ---- */
/* loss[0] = mean((y-t)^2); t = target[i] or the constant `tconst` when target == NULL */
int loans_mse_fwd_f32(const float* y, const float* target, float tconst, float* loss, int32_t n, void* stream);
/* gy[i] = gloss[0] * 2/n * (y-t) */
int loans_mse_bwd_f32(const float* y, const float* target, float tconst, const float* gloss, float* gy,
                      int32_t n, void* stream);
/* kind 0 = DirectionLoss (needs imgH,imgW), 1 = OutOfImageLoss * oob_scale. grid [B][2][th][tw]. */
int loans_grid_loss_fwd_f32(const float* grid, float* loss, int32_t kind, float imgH, float imgW, float oob_scale,
                            int32_t B, int32_t th, int32_t tw, void* stream);
/* ggrid += gloss[0] * dloss/dgrid (touches only the three corner points) */
int loans_grid_loss_bwd_f32(const float* grid, const float* gloss, float* ggrid, int32_t kind,
                            float imgH, float imgW, float oob_scale,
                            int32_t B, int32_t th, int32_t tw, void* stream);

/* ---- VisualBackprop and grayscale rois (insights/visual_backprop.py:16-53; sheep/sheep_localizer.py:65-68,105-108) ---- */
/* out[row] = (1 / cdiv) * sum_c a(x[row][c]); a = identity, or relu(x * scale[c] + shift[c]) when scale / shift are given
 * (F.average(input, axis=1) of a convolution / pooling node's input, visual_backprop.py:39); C % 4 == 0; cdiv = the logical
 * channel count (3 for the 4-channel padded frames) */
int loans_channel_mean_f32(const float* x, const float* scale, const float* shift, float* out, int64_t rows, int32_t C,
                           int32_t cdiv, void* stream);
int loans_channel_mean_bf16(const void* x, const float* scale, const float* shift, float* out, int64_t rows, int32_t C,
                            int32_t cdiv, void* stream);
/* out = deconvolution_2d(feat [B][fh][fw], ones(kh, kw), stride, pad, outsize (H, W)) * avg [B][H][W]   (visual_backprop.py:31-40) */
int loans_vbp_scale_f32(const float* feat, const float* avg, float* out, int32_t B, int32_t fh, int32_t fw, int32_t H, int32_t W,
                        int32_t kh, int32_t kw, int32_t sy, int32_t sx, int32_t ph, int32_t pw, void* stream);
/* per image of n values, in place: (x - min) / (max - min)   (visual_backprop.py:48-52) */
int loans_minmax_normalize_f32(float* x, int32_t B, int32_t n, void* stream);
/* rois NHWC4 -> 0.299 * ch2 + 0.587 * ch1 + 0.114 * ch0 per pixel, and its gradient (sheep_localizer.py:65-68) */
int loans_gray_fwd_f32(const float* rois_nhwc4, float* out, int64_t npix, void* stream);
int loans_gray_bwd_f32(const float* g, float* grois_nhwc4, int64_t npix, void* stream);

/* ---- the imgaug branch of the input pipeline (common/datasets/image_dataset.py:57-70,80-83), one position of the sampled
 * operation order per launch: params_dev [B][8] int32, [0] = op (0 copy, 1 Fliplr, 2 AddToHueAndSaturation: [1] dh [2] ds,
 * 3 CropAndPad: [1..4] top, right, bottom, left pixels (< 0 crop, > 0 pad), [5] fill 0 constant / 1 edge, resized back to H x W);
 * uint8 HWC RGB frames of one size, in != out.  Integer arithmetic throughout (loans_amd/common/datasets/augment.py is the
 * NumPy form of the same operations). */
int loans_augment_stage_u8(const void* in, void* out, int32_t B, int32_t H, int32_t W, const int32_t* params_dev, void* stream);

/* ---- optimiser: chainer.optimizers.Adam(alpha, amsgrad=True) over one flat buffer
 *      (train_sheep_localizer.py:130-134; sheep_updater.py:52,66). lr_t = alpha*sqrt(1-b2^t)/(1-b1^t)
 *      is computed by the caller; eps sits outside the bias correction. grad_scale multiplies g first
 *      (1/world_size after a sum all-reduce). ---- */
int loans_adam_amsgrad_f32(float* p, const float* g, float* m, float* v, float* vhat, int64_t n,
                           double lr_t, double beta1, double beta2, double eps, double eta, double weight_decay_rate,
                           double grad_scale, void* stream);
/* same update with lr_t read from device memory at execution time (one float): the launch is then independent of the
 * step count and can be captured once in a hipGraph; the caller refreshes *lr_t_dev before each replay */
int loans_adam_amsgrad_devlr_f32(float* p, const float* g, float* m, float* v, float* vhat, int64_t n,
                                 const float* lr_t_dev, double beta1, double beta2, double eps, double eta,
                                 double weight_decay_rate, double grad_scale, void* stream);

/* plain Adam -- chainer.optimizers.Adam's default amsgrad=False (train_sheep_localizer.py:130 passes amsgrad=True; the class
 * surface takes both): the same update with sqrt(v) in the denominator, no vhat.  lr_t_dev != NULL: the rate is read from
 * device memory (hipGraph), lr_t is ignored */
int loans_adam_f32(float* p, const float* g, float* m, float* v, int64_t n, double lr_t, const float* lr_t_dev,
                   double beta1, double beta2, double eps, double eta, double weight_decay_rate, double grad_scale,
                   void* stream);

/* chainer.optimizers.MomentumSGD with the WeightDecay hook applied to the gradient first, one launch over a flat range:
 *   g' = g * grad_scale + weight_decay_rate * p;   v = momentum * v - lr * g';   p = p + v
 * lr_dev != NULL: the rate is read from device memory when the kernel runs (hipGraph), lr is ignored.  p, g, v: 16-byte
 * aligned like the Adam entries' buffers (four floats per thread); n need not be a multiple of four. */
int loans_momentum_sgd_f32(float* p, const float* g, float* v, int64_t n, double lr, const float* lr_dev, double momentum,
                           double weight_decay_rate, double grad_scale, void* stream);

/* The same with the weight decay switched off inside marked ranges of the flat buffer (BN scales / shifts, biases).  The ranges
 * are `nseg` segments that tile [0, n): seg_end[s] is segment s's exclusive end -- ascending, no empty segment, every end but the
 * last a multiple of 4 (a float4 never straddles a boundary), the last equal to n --, bit 0 of seg_flags[s] says "exempt from
 * decay".  Inside an exempt segment weight_decay_rate counts as 0, everything else is loans_momentum_sgd_f32's arithmetic bit for
 * bit.  seg_end_dev / seg_flags_dev: the table in DEVICE memory (caller-owned, alive until the launch has run; read into LDS, so
 * nseg <= loans_momentum_sgd_max_segments() = 1024); seg_end_host: the same ends in host memory, checked on every call --
 * LOANS_EINVAL, and no launch, for a table that breaks a rule above, a null pointer or p / g / v off a 16-byte boundary. */
int loans_momentum_sgd_seg_f32(float* p, const float* g, float* v, int64_t n, double lr, const float* lr_dev, double momentum,
                               double weight_decay_rate, double grad_scale, const int64_t* seg_end_dev,
                               const uint8_t* seg_flags_dev, const int64_t* seg_end_host, int32_t nseg, void* stream);
int loans_momentum_sgd_max_segments(void);

/* LARS (You et al. 2017): momentum SGD whose rate is scaled per segment of the flat buffer by a trust ratio.  The segment table is
 * loans_momentum_sgd_seg_f32's (same rules, same checks, nseg <= LOANS_LARS_MAX_SEGMENTS) with a second flag bit:
 *   W_s  = sqrt(sum p_i^2)      G_s = |grad_scale| * sqrt(sum g_i^2)                  over segment s
 *   wd_s = (flags[s] & 1) ? 0 : weight_decay_rate
 *   r_s  = (flags[s] & 2) ? 1 : (W_s > 0 && G_s > 0 ? eta * W_s / (G_s + wd_s * W_s + eps) : 1)
 *   g' = g * grad_scale + wd_s * p;   v = momentum * v - (lr * r_s) * g';   p = p + v
 *
 * loans_lars_ratios_f32: one pass over p and g (two launches: per-unit partial sums of squares, then a per-segment fold) leaves
 * r_s, rounded to fp32 once, in ratios_dev[0 .. nseg) and, if norms_dev != NULL, W_s and G_s in norms_dev[2 s], norms_dev[2 s + 1].
 * Every square and every sum is fp64, the order of the additions is fixed and no atomic is used: the same inputs give the same
 * bits.  Work is cut per segment into units of LOANS_LARS_UNIT floats; seg_first_unit_dev[s] = the sum of
 * ceil(length / LOANS_LARS_UNIT) over the segments before s, in device memory like the ends and flags.  workspace: device
 * memory, 16-byte aligned, of at least loans_lars_workspace_bytes(seg_end_host, nseg) bytes (-1 for a table that breaks a
 * rule); it need not be initialised.  Nothing is synchronised with the host.
 *
 * loans_lars_update_f32: loans_momentum_sgd_seg_f32 with the rate of segment s = fl(fl(lr) * ratios_dev[s]) -- one fp32 product
 * of the rate as the kernel holds it (the argument rounded to fp32, or *lr_dev) --, everything else loans_momentum_sgd_f32's
 * arithmetic bit for bit.
 *
 * LOANS_EINVAL, and no launch: a null pointer (norms_dev may be null), p / g / v / workspace off a 16-byte boundary, n <= 0,
 * nseg outside [1, LOANS_LARS_MAX_SEGMENTS], ends not ascending, an inner end that is no multiple of 4, a last end != n, a
 * workspace that is too small, eta <= 0, eps < 0. */
#define LOANS_LARS_UNIT 4096
#define LOANS_LARS_MAX_SEGMENTS 1024
int64_t loans_lars_workspace_bytes(const int64_t* seg_end_host, int32_t nseg);
int loans_lars_ratios_f32(const float* p, const float* g, int64_t n, double weight_decay_rate, double grad_scale, double eta,
                          double eps, const int64_t* seg_end_dev, const uint8_t* seg_flags_dev, const int64_t* seg_first_unit_dev,
                          const int64_t* seg_end_host, int32_t nseg, float* ratios_dev, double* norms_dev, void* workspace,
                          int64_t workspace_bytes, void* stream);
int loans_lars_update_f32(float* p, const float* g, float* v, int64_t n, double lr, const float* lr_dev, double momentum,
                          double weight_decay_rate, double grad_scale, const int64_t* seg_end_dev, const uint8_t* seg_flags_dev,
                          const float* ratios_dev, const int64_t* seg_end_host, int32_t nseg, void* stream);

/* LAMB (You et al. 2019, algorithm 2 with the identity for phi): Adam's direction with decoupled weight decay, its length set per
 * segment of the flat buffer by the trust ratio.  The segment table is LARS's (same rules, same checks, same two flag bits,
 * LOANS_LARS_UNIT, LOANS_LARS_MAX_SEGMENTS, loans_lars_workspace_bytes).  Step t (1-based):
 *   g^ = g * grad_scale;   m' = m + (1 - beta1) (g^ - m);   v' = v + (1 - beta2) (g^ g^ - v)
 *   a  = (m' c1) / (sqrt(v' c2) + eps)       c1 = 1 / (1 - beta1^t), c2 = 1 / (1 - beta2^t): the caller forms them in double
 *   wd_s = (flags[s] & 1) ? 0 : weight_decay_rate;   u = a + wd_s p
 *   W_s = sqrt(sum p_i^2)   U_s = sqrt(sum u_i^2)    over segment s
 *   r_s = (flags[s] & 2) || W_s == 0 || U_s == 0 ? 1 : W_s / U_s
 *   p' = p - (lr r_s) u
 * fp32 per element with the order fixed by fmaf: m' = fmaf(omb1, g^ - m, m); v' = fmaf(omb2, fmaf(g^, g^, -v), v);
 * u = fmaf(wd_s, p, a); p' = fmaf(-fl(fl(lr) * r_s), u, p); every scalar is rounded to fp32 once.  Squares and sums of the norms
 * are fp64 in a fixed order, r_s is formed in double and rounded to fp32 once; no atomic is used: the same inputs give the same bits.
 *
 * Three launches per step, nothing is synchronised with the host:
 * loans_lamb_moments_f32  reads p (not written), g, m, v; writes m', v' and, per unit of LOANS_LARS_UNIT floats, the sums of p^2
 *                         and u^2 into the workspace (two doubles per unit; it need not be initialised);
 * loans_lamb_ratios_f32   folds the workspace per segment in ascending unit order: r_s into ratios_dev[0 .. nseg) and, if
 *                         norms_dev != NULL, W_s and U_s into norms_dev[2 s], norms_dev[2 s + 1];
 * loans_lamb_update_f32   reads p, m', v', forms u again from them -- the same function, the same bits as the u whose square
 *                         was summed -- and writes p'.  c1, c2, eps and weight_decay_rate must be those of the moments call.
 *
 * LOANS_EINVAL, and no launch: a null pointer (norms_dev may be null), p / g / m / v / workspace off a 16-byte boundary, the
 * int64 tables off an 8-byte one, ratios_dev off a 4-byte one, n <= 0, nseg outside [1, LOANS_LARS_MAX_SEGMENTS], ends not
 * ascending, an inner end that is no multiple of 4, a last end != n, a workspace that is too small, beta1 or beta2 outside
 * [0, 1), c1 or c2 not >= 1, eps < 0. */
int loans_lamb_moments_f32(const float* p, const float* g, float* m, float* v, int64_t n, double beta1, double beta2, double c1,
                           double c2, double eps, double weight_decay_rate, double grad_scale, const int64_t* seg_end_dev,
                           const uint8_t* seg_flags_dev, const int64_t* seg_first_unit_dev, const int64_t* seg_end_host,
                           int32_t nseg, void* workspace, int64_t workspace_bytes, void* stream);
int loans_lamb_ratios_f32(int64_t n, const int64_t* seg_end_dev, const uint8_t* seg_flags_dev, const int64_t* seg_first_unit_dev,
                          const int64_t* seg_end_host, int32_t nseg, float* ratios_dev, double* norms_dev, const void* workspace,
                          int64_t workspace_bytes, void* stream);
int loans_lamb_update_f32(float* p, const float* m, const float* v, int64_t n, double lr, double c1, double c2, double eps,
                          double weight_decay_rate, const int64_t* seg_end_dev, const uint8_t* seg_flags_dev,
                          const float* ratios_dev, const int64_t* seg_end_host, int32_t nseg, void* stream);

/* Gradient clipping by the global L2 norm (chainer.optimizer_hooks.GradientClipping) over the first n floats g of a flat gradient
 * buffer; grad_scale = the optimiser's (1 / world size where the buffer holds the sum over ranks), max_norm = the threshold c > 0:
 *   S    = sum g_i^2                      every g_i converted to double and squared (exact), summed in fp64 in a FIXED order
 *   N    = |grad_scale| * sqrt(S)         in double: the norm of the gradient the optimiser will actually apply
 *   k    = (N is finite and N > c) ? c / N : 1          in double, rounded to fp32 ONCE
 *   g_i' = fl32(g_i * k)                  one fp32 product per element, in place -- skipped entirely when k == 1
 * N == c does not clip (Chainer's `rate < 1`); an all-zero gradient gives N = 0, k = 1 and no division; a non-finite N (a NaN or inf
 * anywhere in g, or a sum that overflows) gives k = 1: g stays bit for bit as it was and the record holds the non-finite N (Chainer
 * would write 0 * inf); max_norm = +inf is legal and means "measure only".
 *
 * loans_grad_norm_f32: two launches -- one fp64 partial per unit of LOANS_LARS_UNIT floats (unit u = floats [4096 u, ..)), then one
 * wave that sums the partials of lane l = l, l + 64, .. in ascending order and the 64 lane sums in an xor butterfly -- leave
 * record_dev[0] = N (rounded to fp32 once) and record_dev[1] = k.  The order of the additions is a function of n alone and no atomic
 * is used: the same inputs give the same bits.  workspace: device memory, 16-byte aligned, of at least
 * loans_grad_clip_workspace_bytes(n) bytes (host arithmetic only; < 0: a LOANS_E* code); it need not be initialised.
 * loans_grad_clip_apply_f32: one launch; every block reads record_dev[1] and returns at once if it is 1, else g *= k in place.
 * Nothing is synchronised with the host.
 *
 * LOANS_EINVAL, and no launch: a null pointer, g or workspace off a 16-byte boundary, record_dev off an 8-byte one, n <= 0, a
 * workspace that is too small, max_norm not > 0 (or NaN), a non-finite grad_scale.  LOANS_ERANGE: n > LOANS_GRAD_CLIP_MAX_N. */
#define LOANS_GRAD_CLIP_MAX_N ((int64_t)1 << 42)
int64_t loans_grad_clip_workspace_bytes(int64_t n);
int loans_grad_norm_f32(const float* g, int64_t n, double grad_scale, double max_norm, void* workspace, int64_t workspace_bytes,
                        float* record_dev /* [0] = N, [1] = k */, void* stream);
int loans_grad_clip_apply_f32(float* g, int64_t n, const float* record_dev, void* stream);

/* Gradient accumulation (train_imagenet.py --accum-steps K): the gradients of K micro-batches summed in an accumulator the size of
 * the gradient arena, one launch per micro-batch over the first n floats of both buffers:
 *   LOANS_ACCUM_STORE:  acc_i = g_i                   the first micro-batch (acc needs no initialisation; g is not written)
 *   LOANS_ACCUM_ADD:    acc_i = fl32(acc_i + g_i)     micro-batches 2 .. K - 1 (g is not written)
 *   LOANS_ACCUM_CLOSE:  g_i   = fl32(acc_i + g_i)     the last one: the sum lands in g, acc is not written
 * The closed gradient is ((g1 + g2) + g3) + .. + gK: one IEEE fp32 addition per element and micro-batch, in that order -- the bits
 * of torch.add, NaN, inf, signed zeros and subnormals included.  No scaling, no fp64, no atomic; floats behind n are not touched.
 * LOANS_EINVAL, and no launch: a null pointer, acc or g off a 16-byte boundary, n <= 0, an unknown mode.  LOANS_ERANGE:
 * n > LOANS_GRAD_CLIP_MAX_N. */
#define LOANS_ACCUM_STORE 0
#define LOANS_ACCUM_ADD 1
#define LOANS_ACCUM_CLOSE 2
int loans_grad_accum_f32(float* acc, float* g, int64_t n, int32_t mode, void* stream);

/* A table of streaming jobs over float ranges in ONE launch: the exponential moving average of a model's weights
 * (loans_amd/runtime/average.py) -- job 0 the whole parameter arena, the others the ~100 small BN statistics tensors.
 *   LOANS_AVG_UPDATE:  dst += omd * (src - dst)      (omd = 1 - decay; exactly nothing where dst == src)
 *   LOANS_AVG_SWAP:    dst <-> src, bit for bit
 * Work is cut into units of LOANS_AVG_UNIT floats: first_unit = the sum of ceil(n / LOANS_AVG_UNIT) over the jobs before it, `units`
 * that sum over all jobs; n need not be a multiple of 4.  dst is streamed (non-temporal), src stays cacheable.  jobs_dev: the table
 * in DEVICE memory (caller-owned, alive until the launch has run); jobs_host: the same table in host memory, checked on every call
 * -- LOANS_EINVAL, and no launch, for a null or not 16-byte aligned dst / src, n <= 0, a first_unit or `units` that is not the sum
 * above, njobs <= 0, a null table or an unknown mode.  Ranges must not overlap. */
#define LOANS_AVG_UNIT 4096
#define LOANS_AVG_UPDATE 0
#define LOANS_AVG_SWAP 1
typedef struct loans_avg_job {
    void* dst;
    void* src;
    int64_t n;
    int64_t first_unit;
} loans_avg_job;
int loans_average_jobs_f32(const loans_avg_job* jobs_dev, const loans_avg_job* jobs_host, int32_t njobs, int64_t units, int32_t mode,
                           float omd, void* stream);

/* ---- input contract on the GPU (common/datasets/image_dataset.py:16-28 `resize_image` -> Pillow
 *      Image.resize(LANCZOS); :98 `image / 255`).  Bit-exact restatement of Pillow's 8-bit two-pass resampler
 *      (libImaging/Resample.c): per output coordinate a window bounds[2*i] = first input index, bounds[2*i+1] = taps, and
 *      ks int32 coefficients in 22-bit fixed point (tables from loans_amd/common/datasets/resample.py); horizontal pass
 *      into tmp [B][inH][outW][3], vertical pass into dst.  src is [B][inH][inW][3] uint8 RGB.
 *      _u8: dst [B][outH][outW][3] uint8;  _u8_f32: dst [B][3][outH][outW] float32 = resized / 255 (the hot path's frames). ---- */
/* A batch of frames of DIFFERENT sizes (the naive crop branch of ImageDataset, image_dataset.py:86-90, gives every frame a
 * size of its own) resized to one outH x outW batch in ONE launch pair.  One job per frame: byte offsets of the frame in
 * `src` ([inH][inW][3] uint8) and of its intermediate in `tmp` ([inH][outW][3]), and the int32-word offsets of ITS coefficient
 * tables in `tables` (per axis: bounds [out][2], coefficients [out][ks]); frame j writes dst[j] ([3][outH][outW] float32 =
 * resized / 255), i.e. the batch is produced in job order.  jobs / tables are device memory; max_inH = the tallest frame.
 * A frame may be stored mirrored (`flip`): the host then stages contiguous rows instead of reversing 3-byte pixels. */
typedef struct loans_resample_job {
    int64_t src_off, tmp_off;
    int32_t inH, inW;
    int32_t hb_off, hk_off, hks;
    int32_t vb_off, vk_off, vks;
    int32_t flip;               /* != 0: the frame is the horizontal mirror of the buffer (random_flip, image_dataset.py:40-44) */
} loans_resample_job;
int loans_resize_ragged_u8_f32(const uint8_t* src, uint8_t* tmp, float* dst, const loans_resample_job* jobs, int32_t njobs,
                               const int32_t* tables, int32_t max_inH, int32_t outH, int32_t outW, void* stream);
int loans_resize_lanczos_u8(const uint8_t* src, uint8_t* tmp, uint8_t* dst, int32_t B, int32_t inH, int32_t inW,
                            int32_t outH, int32_t outW, const int32_t* hbounds, const int32_t* hk, int32_t hks,
                            const int32_t* vbounds, const int32_t* vk, int32_t vks, void* stream);
int loans_resize_lanczos_u8_f32(const uint8_t* src, uint8_t* tmp, float* dst, int32_t B, int32_t inH, int32_t inW,
                                int32_t outH, int32_t outW, const int32_t* hbounds, const int32_t* hk, int32_t hks,
                                const int32_t* vbounds, const int32_t* vk, int32_t vks, void* stream);
/* [B][H][W][3] uint8 -> [B][3][H][W] float32 / 255 (frames that need no resize) */
int loans_u8hwc3_to_f32chw(const uint8_t* src, float* dst, int32_t B, int32_t H, int32_t W, void* stream);

/* ---- crop + resize feed of the ImageNet pre-training arm (csrc/croprs.hip): random-resized-crop / centre crop, i.e.
 *      Image.fromarray(frame[y0:y0+h, x0:x0+w]) [.transpose(FLIP_LEFT_RIGHT)] .resize((outW, outH), Image.BILINEAR) / 255 in
 *      CHW, bit for bit, for a whole batch in ONE launch.  The crop is read IN PLACE: job j names the first byte of its frame
 *      (or of the rows staged for it) in `src`, the row pitch in bytes, and the crop's origin and size in pixels of that
 *      frame; the tables are those of the crop's width and height (`tables` as in loans_resize_ragged_u8_f32: per axis bounds
 *      [out][2] then coefficients [out][ks], offsets in int32 words).  `flip`: crop, mirror, resize -- pixel x of the crop is
 *      pixel x0 + w - 1 - x of the row.  Job j writes dst[j] ([3][outH][outW] float32).  blockIdx.y = the frame, blockIdx.x = a
 *      band of loans_crop_band_rows(outH, outW) output rows; a block runs the horizontal pass over the crop rows its band
 *      needs into LDS (uint8 [rows][outW][3]; static LDS, LOANS_CROP_LDS_BYTES at most -- a smaller image, more blocks per
 *      CU, where max_vks allows it), then the vertical pass out of LDS; a band whose rows do not fit takes several fills.  No intermediate in HBM.  The one shape it cannot do is an output row that
 *      needs more crop rows than fit: LOANS_EINVAL when max_vks (the largest vks of the jobs, from the host) exceeds
 *      LOANS_CROP_LDS_BYTES / (outW * 3), as for null pointers, non-positive sizes and njobs > 65535 -- before any launch.
 *      The jobs themselves are device memory and are NOT checked here: the host wrapper validates them
 *      (loans_amd/common/datasets/crop_resize.py). ---- */
#define LOANS_CROP_LDS_BYTES 65536
typedef struct loans_crop_job {
    int64_t src_off;            /* byte offset in src of pixel (0, 0) of the frame the box refers to */
    int32_t pitch;              /* bytes from one row of that frame to the next (>= 3 * its width) */
    int32_t y0, x0, h, w;       /* the crop, in pixels of that frame */
    int32_t hb_off, hk_off, hks;    /* tables of resample_coeffs(w, outW, 'bilinear') */
    int32_t vb_off, vk_off, vks;    /* tables of resample_coeffs(h, outH, 'bilinear') */
    int32_t flip;
} loans_crop_job;
int loans_crop_resize_u8_f32(const uint8_t* src, float* dst, const loans_crop_job* jobs, int32_t njobs,
                             const int32_t* tables, int32_t max_vks, int32_t outH, int32_t outW, void* stream);
/* The same launch over SEVERAL source buffers (a batch that mixes frames resident in cache slabs with frames uploaded this
 * moment): `srcs` is a DEVICE table of nsrcs base pointers, `src_index` a DEVICE array of njobs entries -- job n's src_off is
 * relative to srcs[src_index[n]]; everything else as above, loans_crop_job unchanged.  A block reads its job's index once and
 * writes nothing where it lies outside [0, nsrcs).  LOANS_EINVAL also for a null table or index array and for nsrcs <= 0. */
int loans_crop_resize_srcs_u8_f32(const uint8_t* const* srcs, const int32_t* src_index, int32_t nsrcs, float* dst,
                                  const loans_crop_job* jobs, int32_t njobs, const int32_t* tables, int32_t max_vks,
                                  int32_t outH, int32_t outW, void* stream);
/* output rows per block of that launch (host arithmetic only; <= 0 for non-positive sizes) */
int loans_crop_band_rows(int32_t outH, int32_t outW);

/* ---- mixup / CutMix of a device batch with a shifted copy of itself (csrc/mix.hip).  x, out: contiguous [B][C][H][W] fp32;
 *      row b's partner is row p = (b - shift) mod B.  Per element of row b
 *        inside the box y0 <= y < y1, x0 <= x < x1      out = x[p]                          (a bit copy)
 *        outside, oml == 0                              out = x[b]                          (a bit copy; the partner is not read)
 *        outside, otherwise                             out = fma(lam, x[b], oml * x[p])    (fp32: two roundings)
 *      mixup: an empty box and (lam, 1 - lam); CutMix: a box and (1, 0); no mixing: an empty box and (1, 0).  One streaming
 *      launch, 16-byte accesses where W % 4 == 0 and both pointers are 16-byte aligned; no atomics: two launches, the same bits.
 *      LOANS_EINVAL -- before any launch -- for a null pointer, out == x (partners are read after they would be written),
 *      non-positive sizes, shift outside [0, B), a box that is not 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W, a non-finite
 *      weight; LOANS_ERANGE for C * H * W >= 2^30 (the batch itself is indexed in 64 bits). ---- */
int loans_batch_mix_f32(const float* x, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                        int32_t shift, float lam, float oml,
                        int32_t y0, int32_t x0, int32_t y1, int32_t x1, void* stream);

/* ---- photometric augmentation of a device batch (csrc/photo.hip): colour jitter, lighting noise, random erasing.  x, out:
 *      contiguous [B][3][H][W] fp32; image n has the job jobs[n].  A pixel's three channels are worked on together, with
 *        grey(r, g, b) = fma(0.299, r, fma(0.587, g, 0.114 * b))
 *        brightness   x = clamp01(b * x)
 *        saturation   x = clamp01(fma(s, x, oms * grey(pixel)))
 *        contrast     x = clamp01(fma(c, x, omc * m)),  m = the image's mean grey as it stands when contrast is reached (after the
 *                     operations that precede contrast in this image's order): fp32 greys summed in fp64 in a fixed order, divided
 *                     by H W in fp64, rounded to fp32 once
 *      in the order `order` names: 0 BCS, 1 BSC, 2 CBS, 3 CSB, 4 SBC, 5 SCB.  A factor that is exactly 1 skips its operation (no
 *      clamp: a bit copy).  Then, if any addend is non-zero, x = x + add[channel], no clamp; last, every pixel inside the erase box
 *      y0 <= y < y1, x0 <= x < x1 becomes fill[channel], a bit copy.  All factors 1, a zero addend, an empty box: the image leaves
 *      bit for bit.  omc = fl32(1 - c) and oms = fl32(1 - s) are rounded once, by the caller.  Hue is not built.
 *      loans_photo_grey_means_f32: for the images with c != 1, one fp64 partial sum per (image, block) into `workspace` (device
 *      memory, 8-byte aligned, loans_photo_workspace_bytes(B, H, W) bytes at least; it need not be initialised), then a small
 *      launch that folds each image's partials in ascending block order and leaves its fp32 mean behind the partials; no atomics;
 *      no launch when no image has c != 1.  loans_photo_apply_f32: one streaming launch that reads those means from the same
 *      workspace; out == x is allowed (every lane owns its pixels in all three planes); 16-byte accesses where
 *      W % 4 == 0 and x and out are 16-byte aligned.  `workspace` may be null for it when no image has c != 1.  Two runs give the
 *      same bits.  jobs_dev: the table in DEVICE memory; jobs_host: the same table in host memory, checked on every call.
 *      LOANS_EINVAL -- before any launch -- for a null or misaligned pointer, non-positive sizes, C != 3, a workspace that is too
 *      small, a non-finite factor, addend or fill, an order outside [0, 5], a box that is not 0 <= y0 <= y1 <= H, 0 <= x0 <= x1
 *      <= W; LOANS_ERANGE for 3 * H * W >= 2^30 (the batch itself is indexed in 64 bits).  Nothing is synchronised with the host. ---- */
typedef struct loans_photo_job {
    float b, c, s;              /* the three factors */
    float omc, oms;             /* fl32(1 - c), fl32(1 - s) */
    int32_t order;              /* 0 .. 5: the permutation of (brightness, contrast, saturation) */
    float add[3];               /* RGB addend (lighting noise) */
    int32_t y0, x0, y1, x1;     /* the erase box; empty where y1 <= y0 or x1 <= x0 */
    float fill[3];              /* what an erased pixel becomes */
} loans_photo_job;
int64_t loans_photo_workspace_bytes(int32_t B, int32_t H, int32_t W);
int loans_photo_grey_means_f32(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, const loans_photo_job* jobs_dev,
                               const loans_photo_job* jobs_host, void* workspace, int64_t workspace_bytes, void* stream);
int loans_photo_apply_f32(const float* x, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                          const loans_photo_job* jobs_dev, const loans_photo_job* jobs_host, const void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ---- RandAugment / TrivialAugmentWide on a device batch (csrc/randaug.hip; the fourteen operations and their arithmetic are listed
 *      in that file's header and stated in loans_amd/common/datasets/rand_augment.py).  x, out: contiguous [B][3][H][W] fp32; image
 *      n runs the `layers` (1 .. 4) layers of jobs[n] one behind the other.  Per layer l: op[l] 0 .. 13 (Identity, ShearX, ShearY,
 *      TranslateX, TranslateY, Rotate, Brightness, Color, Contrast, Sharpness, Posterize, Solarize, AutoContrast, Equalize);
 *      a[l]: for ops 1 .. 5 the six 16.16 fixed-point coefficients of the output -> input map, xin = (a0 x + a1 y + a2) >> 16,
 *      yin = (a3 x + a4 y + a5) >> 16 (|a0|, |a1|, |a3|, |a4| <= 2^20, |a2|, |a5| <= 2^50), for Posterize a[l][0] = the bits kept, 2 .. 8;
 *      f[l]: for ops 6 .. 9 the factor and fl32(1 - factor), rounded once by the caller, for Solarize f[l][0] = the threshold.  `fill`
 *      is what a pixel becomes whose source lies outside the frame.  A layer that is the identity for its image leaves it bit for bit.
 *      `workspace`: device memory, 16-byte aligned, loans_ra_workspace_bytes(B, H, W) bytes at least (block records, folded records,
 *      one scratch batch); it need not be initialised.  loans_ra_stats_f32: the statistics of layer `layer` (0 .. 3) of the batch x as
 *      it stands -- the grey mean for Contrast, the channel extremes for AutoContrast, the channel histograms for Equalize -- folded
 *      in a fixed order into the workspace; no floating-point atomics; no launch when no image's layer needs one.
 *      loans_ra_apply_f32: the whole stage, per layer the statistics step where an image needs it and one apply launch; the result ends
 *      in out, which may be x; x is only read where out is another tensor (neither may overlap the workspace).  Two runs give the same
 *      bits.  jobs_dev: the table in DEVICE memory; jobs_host: the same table in host memory, checked on every call.  LOANS_EINVAL --
 *      before any launch -- for a null or misaligned pointer (4 bytes for x / out, 8 for the tables, 16 for the workspace),
 *      non-positive sizes, C != 3, a workspace that is too small, a layer count outside [1, 4], an unknown operation, a coefficient
 *      beyond the limits, a non-finite factor, threshold or fill, bits outside [2, 8]; LOANS_ERANGE for 3 * H * W >= 2^30 (the batch
 *      itself is indexed in 64 bits).  Nothing is synchronised with the host. ---- */
typedef struct loans_ra_job {
    int64_t a[4][6];            /* per layer: fixed-point coefficients (ops 1 .. 5), or the bits in a[l][0] (Posterize) */
    float f[4][2];              /* per layer: factor and fl32(1 - factor) (ops 6 .. 9), or the threshold in f[l][0] (Solarize) */
    int32_t op[4];              /* per layer: the operation, 0 .. 13 */
    int32_t layers;             /* 1 .. 4 */
    float fill[3];              /* RGB of a pixel whose source lies outside the frame */
} loans_ra_job;
int64_t loans_ra_workspace_bytes(int32_t B, int32_t H, int32_t W);
int loans_ra_stats_f32(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, const loans_ra_job* jobs_dev,
                       const loans_ra_job* jobs_host, int32_t layer, void* workspace, int64_t workspace_bytes, void* stream);
int loans_ra_apply_f32(const float* x, float* out, int32_t B, int32_t C, int32_t H, int32_t W, const loans_ra_job* jobs_dev,
                       const loans_ra_job* jobs_host, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- stochastic depth at a residual unit's junction (csrc/bn_pool.hip; torchvision's StochasticDepth(mode='row') = timm's
 *      drop_path).  The tensors are [B][rows_per_sample][C] (NHWC, rows_per_sample = Ho * Wo); r: B floats in device memory, 0 for a
 *      dropped sample, 1 / (1 - p) for a kept one.  Relu and sign bits (loans_bn_apply_bits_*'s layout, one byte per four channels)
 *      always.
 *      loans_bn_apply_rows_*: y = relu(r[b] (x scale + shift) + second), second = x2 (mode 1) or x2 scale2 + shift2 (mode 2); a
 *      sample with r[b] == 0 is relu(second) to the bit.
 *      loans_bn_bwd_reduce_rows_*: with g = gy * bit, sums fp64 [replicas][2][C] = [sum r g | sum r g xhat], dual (x2 given)
 *      [replicas][4][C] = [sum r g | sum r g xhat | sum g | sum g xhat2], zeroed by the caller: loans_bn_bwd_reduce_rep_*'s layout,
 *      summed by loans_bn_bwd_coeffs_rep_f32 (centred = 0).
 *      loans_bn_bwd_apply_rows_*: gx = k1 (r[b] g) + k2 x + k3, and with x2: gx2 = k1b g + k2b x2 + k3b.
 *      Channel counts: C / V units per row (V = 4 fp32 / 8 bf16 channels) a divisor of 256 or a multiple of it, else LOANS_EINVAL;
 *      LOANS_ERANGE for a sample of 2^30 units or more.  No floating-point atomics but the reduction's fp64 ones. ---- */
int loans_bn_apply_rows_f32(const float* x, const float* scale, const float* shift, const float* x2, const float* scale2,
                            const float* shift2, const float* r, float* y, uint8_t* signbits, int32_t B, int64_t rows_per_sample,
                            int32_t C, int32_t mode, void* stream);
int loans_bn_apply_rows_bf16(const void* x, const float* scale, const float* shift, const void* x2, const float* scale2,
                             const float* shift2, const float* r, void* y, uint8_t* signbits, int32_t B, int64_t rows_per_sample,
                             int32_t C, int32_t mode, void* stream);
int loans_bn_bwd_reduce_rows_f32(const float* gy, const uint8_t* signbits, const float* r, const float* x, const float* mean,
                                 const float* rstd, const float* x2, const float* mean2, const float* rstd2, double* sums,
                                 int32_t replicas, int32_t B, int64_t rows_per_sample, int32_t C, void* stream);
int loans_bn_bwd_reduce_rows_bf16(const void* gy, const uint8_t* signbits, const float* r, const void* x, const float* mean,
                                  const float* rstd, const void* x2, const float* mean2, const float* rstd2, double* sums,
                                  int32_t replicas, int32_t B, int64_t rows_per_sample, int32_t C, void* stream);
int loans_bn_bwd_apply_rows_f32(const float* gy, const uint8_t* signbits, const float* r, const float* x, const float* k1,
                                const float* k2, const float* k3, float* gx, const float* x2, const float* k1b, const float* k2b,
                                const float* k3b, float* gx2, int32_t B, int64_t rows_per_sample, int32_t C, void* stream);
int loans_bn_bwd_apply_rows_bf16(const void* gy, const uint8_t* signbits, const float* r, const void* x, const float* k1,
                                 const float* k2, const float* k3, void* gx, const void* x2, const float* k1b, const float* k2b,
                                 const float* k3b, void* gx2, int32_t B, int64_t rows_per_sample, int32_t C, void* stream);

/* library / build identification */
const char* loans_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LOANS_HIP_H */
