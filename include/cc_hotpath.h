/* cc_hotpath.h — C ABI of the MI355X-native cosmos-curate hot path.
 *
 * One shared library (libcchot.so, built from cosmos_curate_amd/csrc/ by
 * hipcc for gfx950) exporting the functionality the reference obtains from
 * external native libraries.  Each entry point cites
 * the reference interface it replaces (file:line relative to
 * /root/reference/cosmos_curate/).  Plain pointers + sizes only; device
 * memory is referenced by raw HIP device pointers allocated either by the
 * caller's framework (torch) or by cc_malloc below; `stream` arguments are
 * hipStream_t handles passed as uint64 (0 = default stream).
 *
 * Host-side entry points (cc_demux_*) never touch the GPU and work in a
 * GPU-less container; every cc_* device function requires a visible GPU and
 * fails with CC_ERR_HIP otherwise (no CPU fallback anywhere).
 *
 * Errors: every function returns 0 on success or a negative CC_ERR_* code;
 * cc_last_error() returns a thread-local message for the last failure.
 * Thread-safety: handles are single-threaded; distinct handles independent.
 */

#ifndef CC_HOTPATH_H
#define CC_HOTPATH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  CC_OK = 0,
  CC_ERR_INVALID = -1,     /* bad argument */
  CC_ERR_PARSE = -2,       /* malformed container */
  CC_ERR_NOMEM = -3,
  CC_ERR_HIP = -4,         /* HIP runtime failure (incl. no GPU) */
  CC_ERR_NO_ROCDECODE = -5,/* VCN decode library not present at runtime */
  CC_ERR_UNSUPPORTED = -6,
};

const char* cc_last_error(void);

/* ---- version / capability probes ---------------------------------- */
/* Returns CC_OK when a HIP device is visible and usable. */
int cc_hip_available(void);
/* Returns CC_OK when librocdecode can be dlopened (VCN decode usable). */
int cc_rocdecode_available(void);

/* ---- host MP4 demux ------------------------------------------------
 * Replaces PyNvDemuxer (nvcodec_utils.py:224, fps at :124) and is the PTS
 * source behind get_video_timestamps (pipelines/video/utils/
 * decoder_utils.py:230-278).  Pure host C++; no codec work. */
typedef struct cc_demux cc_demux_t;

typedef struct cc_video_info {
  uint32_t width, height;
  uint32_t timescale;
  uint32_t num_samples;
  uint32_t num_sync_samples;
  int32_t  codec;           /* 0 = h264(avc1/avc3), 1 = hevc(hvc1/hev1) */
  double   duration_s;      /* track media duration in seconds */
  double   avg_fps;         /* num_samples / duration */
} cc_video_info;

int  cc_demux_open(const uint8_t* data, size_t size, cc_demux_t** out);
int  cc_demux_probe(const cc_demux_t* d, cc_video_info* info);
/* Sorted presentation timestamps in seconds, float32 — the exact
 * get_video_timestamps contract (decoder_utils.py:275-278).  `cap` is the
 * capacity of `out`; *n gets the sample count. */
int  cc_demux_timestamps(const cc_demux_t* d, float* out, size_t cap, size_t* n);
/* AnnexB packet for sample `index` (decode order): start-code NALs, with
 * SPS/PPS prefixed on sync samples.  Buffer owned by the demuxer, valid
 * until the next cc_demux_packet call or close. */
int  cc_demux_packet(cc_demux_t* d, size_t index, const uint8_t** pkt,
                     size_t* size, int64_t* pts, int32_t* keyframe);
void cc_demux_close(cc_demux_t* d);
/* Sample-exact stream-copy remux of the presentation span [start_s, end_s)
 * into a standalone MP4 (replaces the per-clip ffmpeg re-encode,
 * clip_extraction_stages.py:317-441; DESIGN.md "transcode").  Fails with
 * CC_ERR_UNSUPPORTED when the span's first sample is not a sync sample.
 * *out is malloc'd; free with cc_buffer_free. */
int  cc_demux_remux_clip(cc_demux_t* d, double start_s, double end_s,
                         uint8_t** out, size_t* out_size);
void cc_buffer_free(void* p);

/* ---- device memory (library-owned buffers; callers may also pass
 * torch-allocated device pointers to the kernels below) ---------------- */
int cc_malloc(void** dptr, size_t bytes);
int cc_free(void* dptr);
int cc_memcpy_h2d(void* dst, const void* src, size_t bytes, uint64_t stream);
int cc_memcpy_d2h(void* dst, const void* src, size_t bytes, uint64_t stream);
int cc_stream_sync(uint64_t stream);

/* ---- VCN hardware decode (rocDecode, runtime-probed) ----------------
 * Replaces NVDEC via PyNvVideoCodec CreateDecoder/Decode
 * (nvcodec_utils.py:199-313).  Fails with CC_ERR_NO_ROCDECODE when
 * librocdecode.so is absent (this image ships none; the ABI is the seam). */
typedef struct cc_decode cc_decode_t;
/* codec: 0 = h264, 1 = hevc (cc_video_info.codec values). */
int  cc_decode_session_create(int device, int32_t codec, cc_decode_t** out);
/* One AnnexB access unit (cc_demux_packet output) per call; pkt == NULL
 * flushes the stream (end-of-stream). */
int  cc_decode_submit(cc_decode_t* s, const uint8_t* pkt, size_t size, int64_t pts);
/* Mapped NV12 (8-bit) or P016 (10/12-bit) surfaces land as {y_ptr, uv_ptr,
 * pitch} triples (HIP device pointers into the decoder's surface pool;
 * pitch in bytes, shared by both planes).  Surfaces stay valid until
 * cc_decode_recycle; consume them (launch + synchronize) first. */
typedef struct cc_nv12_frame {
  void* y; void* uv; size_t pitch; int64_t pts; uint32_t width, height;
} cc_nv12_frame;
int  cc_decode_map_frames(cc_decode_t* s, cc_nv12_frame* out, size_t cap, size_t* n);
/* What the stream's sequence header signalled (PyNvVideoCodec exposes the
 * same through the decoder's format query, nvcodec_utils.py:199-313).
 * 8-bit streams are mapped as NV12 surfaces (bytes_per_sample 1), 10- and
 * 12-bit streams as P016 (u16 samples, MSB-aligned, bytes_per_sample 2);
 * cc_nv12_frame keeps its layout for both and `pitch` stays in BYTES.
 * chroma_format: 1 = 4:2:0 (rocDecVideoChromaFormat values).
 * matrix_coefficients: the H.273 code (1 BT.709, 5/6 BT.601, 9 BT.2020-NCL,
 * 2 unspecified); full_range: video_full_range_flag.  Valid after the
 * first sequence callback (i.e. once a submit has reached the SPS);
 * CC_ERR_INVALID before that. */
typedef struct cc_stream_format {
  int32_t bit_depth, chroma_format, matrix_coefficients, full_range,
      bytes_per_sample;
} cc_stream_format;
int  cc_decode_stream_format(const cc_decode_t* s, cc_stream_format* out);
/* The rest of the sequence header's video_signal_description, kept out of
 * cc_stream_format so that struct keeps its layout: the H.273
 * transfer_characteristics (16 = SMPTE ST 2084 PQ, 18 = HLG, 1 = BT.709,
 * 2 unspecified) and colour_primaries (9 = BT.2020) codes.  Either pointer
 * may be NULL.  Valid when cc_decode_stream_format is. */
int  cc_decode_stream_transfer(const cc_decode_t* s,
                               int32_t* transfer_characteristics,
                               int32_t* colour_primaries);
/* Return every surface handed out by map_frames to the decoder pool
 * (rocDecParserMarkFrameForReuse).  Call after the consuming kernels
 * complete. */
int  cc_decode_recycle(cc_decode_t* s);
void cc_decode_destroy(cc_decode_t* s);

/* ---- fused pixel kernels (hand-written HIP, gfx950) -----------------
 * Replace cvcuda.cvtcolor_into(YUV2RGB_NV12) (nvcodec_utils.py:178),
 * cvcuda.resize_into(LINEAR) (:189-194), cvcuda.reformat_into (:267),
 * cv2 INTER_CUBIC (decoder_utils.py:666-670) and the CLIP/torchvision
 * normalize chain (models/clip.py:48-62).  Batched NHWC u8 layouts. */

/* NV12 (Y plane + interleaved UV half-res plane, same pitch) ->
 * RGB888 NHWC at (out_h,out_w) via bilinear taps in converted-RGB space
 * (each tap converted BT.601 limited-range and rounded to u8 first —
 * bit-identical to convert-then-resize, fused to skip the intermediate).
 * This and cc_nv12_to_rgb are cc_yuv420sp_to_rgb[_resize] at (8, 0, 0):
 * one launcher, the same kernels; only the timing names differ
 * ("nv12_to_rgb_resize", "nv12_to_rgb").  CC_ERR_INVALID on null pointers,
 * non-positive sizes, odd h/w or pitch < w. */
int cc_nv12_to_rgb_resize(const void* y, const void* uv, int n,
                          int src_h, int src_w, size_t pitch,
                          void* out_rgb, int out_h, int out_w,
                          uint64_t stream);
/* Plain NV12 -> RGB888 full resolution (the cvtcolor_into twin). */
int cc_nv12_to_rgb(const void* y, const void* uv, int n,
                   int h, int w, size_t pitch, void* out_rgb, uint64_t stream);
/* 8/10/12-bit 4:2:0 semi-planar -> RGB888 NHWC at full resolution with a
 * selectable matrix and range: the cvcuda.cvtcolor_into(YUV2RGB_NV12) call
 * (nvcodec_utils.py:178) for surfaces and colour standards that fixed
 * 8-bit BT.601 conversion cannot express.
 *   bit_depth   8 = u8 samples (NV12); 10 | 12 = u16 samples, MSB-aligned
 *               (P016, what rocDecode emits; the low 16-depth bits are
 *               ignored)
 *   matrix      0 = BT.601, 1 = BT.709, 2 = BT.2020-NCL
 *   full_range  0 = limited (16..235 / 16..240 scaled), 1 = full
 * Frame f's Y plane starts at y + f*pitch_bytes*h, its UV plane at
 * uv + f*pitch_bytes*(h/2).  f32 arithmetic, bit-exact vs tests/yuv_ref.py;
 * (8, 0, 0) is what cc_nv12_to_rgb runs.  Planes and pitch that
 * are 16-byte aligned take the vectorised path (8 pixels per lane);
 * anything else, and w % 8 row tails, a scalar one.  CC_ERR_INVALID on odd
 * h/w, out-of-set bit_depth/matrix/full_range, pitch_bytes <
 * w*bytes_per_sample, an odd pitch or pointer at 16 bit, null pointers or
 * non-positive sizes — before any launch. */
int cc_yuv420sp_to_rgb(const void* y, const void* uv, int n, int h, int w,
                       size_t pitch_bytes, int bit_depth, int matrix,
                       int full_range, void* out_rgb, uint64_t stream);
/* The same conversion fused with the bilinear resize
 * (cvcuda.resize_into(LINEAR), nvcodec_utils.py:189-194): each of the four
 * taps is converted and rounded to u8 first — bit-identical to
 * cc_yuv420sp_to_rgb followed by cc_resize_bilinear_u8; (8, 0, 0) is what
 * cc_nv12_to_rgb_resize runs. */
int cc_yuv420sp_to_rgb_resize(const void* y, const void* uv, int n,
                              int src_h, int src_w, size_t pitch_bytes,
                              int bit_depth, int matrix, int full_range,
                              void* out_rgb, int out_h, int out_w,
                              uint64_t stream);
/* ---- PQ (HDR10) -> SDR tone mapping in the same conversion ------------
 * No counterpart in the reference (cvcuda's conversion is fixed), opt-in
 * like the matrix choice above.  For streams whose transfer function is
 * SMPTE ST 2084 (H.273 transfer_characteristics 16) the R'G'B' values are
 * PQ code values, not gamma-encoded ones; these entries put the chain below
 * between the matrix and the u8 result.  With r8, g8, b8 the three f32
 * values cc_yuv420sp_to_rgb rounds to u8 (8-bit scale at any depth), every
 * step f32 and in this order, bit-exact vs tests/hdr_ref.py:
 *   L   = tin[clamp(floor(c8*16 + 0.5), 0, 4080)]   per channel: inverse PQ
 *         over reference white, on the 12-bit grid of the 8-bit scale
 *   BT.2020 -> BT.709 linear (BT.2087): rows (1.6605, -0.5876, -0.0728),
 *         (-0.1246, 1.1329, -0.0083), (-0.0182, -0.1006, 1.1187), each
 *         (m0*R + m1*G) + m2*B, then max(., 0)
 *   m   = max(max(r, g), b);  s = (1 + m*inv_w2) / (1 + m);
 *   c   = min(c*s, 1)                   extended Reinhard on max-RGB: a
 *                                       pixel at peak maps to 1
 *   out = tout[floor(sqrt(sqrt(c))*4095 + 0.5)]     inverse BT.1886, 2.4
 * with correctly rounded division and square roots.  The two tables carry
 * every transcendental step, so no device pow enters the result.
 *
 * cc_hdr_tables_build writes the CC_HDR_TABLE_BYTES image the kernels read:
 * f32 tin[4096], tin[i] = PQ_EOTF(i/4080) nits / reference_white_nits for
 * i <= 4080 and 0 above, then u8 tout[4096], tout[j] =
 * floor(255*(j/4095)^(4/2.4) + 0.5); computed in double, rounded once.
 * Host-only, touches no device.  transfer: CC_HDR_TRANSFER_PQ; anything
 * else CC_ERR_UNSUPPORTED.  CC_ERR_INVALID on a null pointer or a
 * reference white that is not positive and finite (BT.2408: 203). */
enum { CC_HDR_TRANSFER_PQ = 1 };
#define CC_HDR_TABLE_BYTES 20480
int cc_hdr_tables_build(int transfer, float reference_white_nits,
                        void* host_out);
/* cc_yuv420sp_to_rgb[_resize] with the chain above.  tables_dev: a device
 * copy of the cc_hdr_tables_build image, 16-byte aligned; inv_w2 =
 * 1/(peak_nits/reference_white_nits)^2 as f32.  Same arguments, layouts,
 * alignment rules and checks as the SDR entries; a null or misaligned
 * tables_dev or an inv_w2 that is negative or not finite is CC_ERR_INVALID
 * as well, before any launch.  The fused resize converts each of the four taps to u8 by
 * the full chain before the blend: bit-identical to cc_yuv420sp_hdr_to_rgb
 * followed by cc_resize_bilinear_u8.  Timed as "yuv420sp_hdr_to_rgb" and
 * "yuv420sp_hdr_to_rgb_resize". */
int cc_yuv420sp_hdr_to_rgb(const void* y, const void* uv, int n, int h, int w,
                           size_t pitch_bytes, int bit_depth, int matrix,
                           int full_range, const void* tables_dev,
                           float inv_w2, void* out_rgb, uint64_t stream);
int cc_yuv420sp_hdr_to_rgb_resize(const void* y, const void* uv, int n,
                                  int src_h, int src_w, size_t pitch_bytes,
                                  int bit_depth, int matrix, int full_range,
                                  const void* tables_dev, float inv_w2,
                                  void* out_rgb, int out_h, int out_w,
                                  uint64_t stream);
/* u8 NHWC bilinear resize (cvcuda LINEAR semantics). */
int cc_resize_bilinear_u8(const void* in, int n, int src_h, int src_w,
                          void* out, int dst_h, int dst_w, uint64_t stream);
/* u8 NHWC bicubic resize, A=-0.75 (cv2 INTER_CUBIC semantics). */
int cc_resize_bicubic_u8(const void* in, int n, int src_h, int src_w,
                         void* out, int dst_h, int dst_w, uint64_t stream);
/* ---- antialiased separable resize + crop ----
 * torchvision's Resize(size, BICUBIC | BILINEAR, antialias=True) followed by
 * CenterCrop, computing only the cropped region; written definition and
 * bit-exact reference: tests/resize_aa_ref.py.
 *
 * cc_resize_aa_table_build writes one axis' table for the outputs
 * [crop_off, crop_off + crop_len) of an in_size -> out_size resize, by
 * torch's _compute_indices_min_size_weights_aa (align_corners=False), in
 * double with each weight rounded to f32 once:
 *   scale = in/out; support = (interp/2)*scale if scale >= 1 else interp/2
 *   (interp 4 bicubic, 2 bilinear); taps = 2*ceil(support) + 1;
 *   center = scale*(i + 0.5); first = max(int(center - support + 0.5), 0);
 *   count = min(int(center + support + 0.5), in) - first;
 *   w[j] = filter((j + first - center + 0.5)*invscale) / sum.
 * bicubic uses A = -0.5 (torch's antialias value).  Layout: int32
 * first[crop_len], int32 count[crop_len], f32 w[crop_len][taps], weights
 * past count zero.  Host-only, touches no device.  Returns the image's size
 * in bytes (positive) and *taps; with host_out == NULL it only does that.
 * CC_ERR_INVALID on an unknown filter, non-positive sizes, a crop outside
 * [0, out_size] or a buffer smaller than the image. */
enum { CC_RESIZE_AA_BILINEAR = 0, CC_RESIZE_AA_BICUBIC = 1 };
#define CC_RESIZE_AA_MAX_TAPS 129
int cc_resize_aa_table_build(int filter, int in_size, int out_size,
                             int crop_off, int crop_len, void* host_out,
                             size_t host_out_bytes, int* taps);
/* u8 NHWC (n, src_h, src_w, 3) -> u8 NHWC (n, out_h, out_w, 3) through two
 * device copies of such tables (4-byte aligned; table_y for out_h rows,
 * table_x for out_w columns).  Per output and channel, f32, multiply then
 * add without contraction, k ascending from 0.0f:
 *   hrow[y] = sum_k wx[ox][k] * float(src[y][firstx[ox] + k])
 *   v       = sum_k wy[oy][k] * hrow[firsty[oy] + k]
 *   out     = u8(rintf(min(max(v, 0), 255)))        (half to even)
 * The kernel is the same for every filter and every tap count up to
 * CC_RESIZE_AA_MAX_TAPS (bicubic down to 1/32): horizontal sums are staged
 * in LDS per band of output rows, in as many chunks of source rows as the
 * band needs.  The launcher cannot read the tables, so the kernel does not
 * trust them: it clamps first to [0, src] and count to [0, min(taps, src -
 * first)] where it reads them, which leaves a table of the builder's as it
 * is and keeps any other inside the source.  Before any launch:
 * CC_ERR_INVALID on null or misaligned pointers and non-positive sizes or
 * taps, CC_ERR_UNSUPPORTED on taps above CC_RESIZE_AA_MAX_TAPS or more than
 * 2^31-1 workgroups.  Timed as "resize_aa_u8". */
int cc_resize_aa_u8(const void* in, int n, int src_h, int src_w, void* out,
                    int out_h, int out_w, const void* table_y_dev, int taps_y,
                    const void* table_x_dev, int taps_x, uint64_t stream);
/* (N,H,W,3) u8 -> (N,3,H,W) normalized ((x/255)-mean)/std.
 * out_dtype: 0 = f32, 1 = bf16. */
int cc_clip_preprocess(const void* in, int n, int h, int w,
                       const float mean[3], const float stdev[3],
                       void* out, int out_dtype, uint64_t stream);
/* Normalize + patch-extraction fused: u8 NHWC frames -> the ViT patch
 * GEMM's A layout [n*(h/patch)*(w/patch), kpad] bf16, col order
 * c*P*P + ky*P + kx (conv-weight flatten), zero-padded to kpad (64-
 * multiple).  Replaces the torch reshape/permute/pad chain after
 * cc_clip_preprocess. */
int cc_clip_preprocess_patches(const void* in, int n, int h, int w, int patch,
                               int kpad, const float mean[3],
                               const float stdev[3], void* out,
                               uint64_t stream);
/* Gather + duplicate-count broadcast of selected frames on device
 * (the decode loop's count broadcast, decoder_utils.py:447-453). */
int cc_gather_frames_u8(const void* frames, int n_in, size_t frame_bytes,
                        const int32_t* idx, const int32_t* counts, int n_idx,
                        int total_out, void* out, uint64_t stream);

/* ---- block-matching motion estimation (hand-written HIP, gfx950) ------
 * Replaces the motion-vector source of the motion filter, decode_for_motion
 * (pipelines/video/filtering/motion/motion_vector_backend.py:169-250), which
 * reads vectors from the H.264 decoder's side data; rocDecode exposes none,
 * so the per-block displacement field is estimated from luma instead.
 * Full-search, full-pel, 16x16 blocks, `n` independent (cur, ref) luma
 * pairs per launch: pair f reads cur + f*frame_stride_bytes and
 * ref + f*frame_stride_bytes, rows pitch_bytes apart.  cur and ref may
 * point into one allocation (consecutive frames: cur = ref + one frame).
 * All-integer arithmetic, bit-exact vs tests/motion_est_ref.py:
 *   Y8(s)  = s (bytes_per_sample 1) | s >> 8 (2: P016, MSB-aligned LE)
 *   grid   nby = ceil(h/16), nbx = ceil(w/16)
 *   C(y,x) = Y8(cur[min(y,h-1)][min(x,w-1)])
 *   R(y,x) = Y8(ref[clamp(y,0,h-1)][clamp(x,0,w-1)])
 *   SAD    = sum over the block's 16x16 (j,i) of
 *            |C(16by+j, 16bx+i) - R(16by+j+dy, 16bx+i+dx)|
 *   cost   = SAD + lambda*(|dx|+|dy|), dx,dy in [-search_range, search_range]
 *   winner = lexicographic minimum of (cost, dx*dx+dy*dy, dy, dx)
 * mv_out   int16  [n][nby][nbx][2] = the winner's (dx, dy)
 * cost_out uint32 [n][nby][nbx]    = its cost; may be NULL
 * No alignment beyond the sample size is assumed of cur, ref or the pitch.
 * Before any launch: CC_ERR_INVALID on null cur/ref/mv_out, non-positive
 * n/h/w, search_range outside 1..32, lambda outside 0..255,
 * bytes_per_sample not 1 or 2, pitch_bytes < w*bytes_per_sample,
 * frame_stride_bytes < pitch_bytes*h, an odd pitch, stride or pointer at
 * 2 bytes per sample, mv_out not 2-byte or cost_out not 4-byte aligned;
 * CC_ERR_UNSUPPORTED when the block grid does not fit one launch (more than
 * 65535 block rows or pairs, or 2^24 blocks in all). */
int cc_motion_estimate(const void* cur, const void* ref, int n, int h, int w,
                       size_t pitch_bytes, size_t frame_stride_bytes,
                       int bytes_per_sample, int search_range, int lambda,
                       void* mv_out, void* cost_out, uint64_t stream);

/* ---- ViT MFMA GEMMs -------------------------------------------------
 * Replace the cuBLAS GEMMs under CLIPModel.get_image_features
 * (models/clip.py:71): patch-embed-as-GEMM, QKV/out projections, MLP.
 * C[M,N] = A[M,K] (bf16, row-major) x B[N,K]^T (bf16, row-major "weight
 * layout") + bias[N] (f32, optional NULL).  c_dtype: 0 = f32, 1 = bf16. */
int cc_gemm_bf16(const void* A, const void* B, void* C,
                 int64_t M, int64_t N, int64_t K,
                 const float* bias, int c_dtype, uint64_t stream);
/* Fused-epilogue form: act 0 = none, 1 = quick-gelu (x*sigmoid(1.702x),
 * the CLIP MLP activation), 2 = tanh-gelu (SigLIP), 3 = erf-gelu
 * (0.5x(1 + erf(x/sqrt 2)), torch gelu approximate="none"; InternVideo2);
 * residual (bf16 [M,N], may be NULL) is added after the activation — fuses
 * the MLP/attention elementwise kernels into the producing GEMM (DESIGN.md
 * §3).  No other act value is taken: CC_ERR_INVALID, in every entry with
 * an act argument.  act 3 is instantiated with a bias and without a
 * residual (an fc1); any other act-3 call returns CC_ERR_UNSUPPORTED. */
int cc_gemm_bf16_ex(const void* A, const void* B, void* C,
                    int64_t M, int64_t N, int64_t K,
                    const float* bias, int c_dtype, int act,
                    const void* residual, uint64_t stream);
/* Row-strided form: A row i starts at A + i*lda, residual row i at
 * residual + i*ldr (elements; C stays dense [M,N]).  Lets the last
 * encoder layer of a CLS-pooled tower (the hidden_states[:, 0] pooling
 * under models/clip.py:71) run its Q projection and out-proj on the CLS
 * rows of a [frames*seq, hidden] tensor in place, with no gather copy.
 * lda >= K, lda % 8 == 0 (16-byte direct-to-LDS loads), ldr >= N; ldr is
 * ignored when residual is NULL.  Strided launches run the 128-tile
 * body; lda == K and ldr == N behaves exactly as cc_gemm_bf16_ex. */
int cc_gemm_bf16_strided(const void* A, int64_t lda, const void* B, void* C,
                         int64_t M, int64_t N, int64_t K, const float* bias,
                         int c_dtype, int act, const void* residual,
                         int64_t ldr, uint64_t stream);

/* How a cc_gemm_bf16* call with these arguments would be launched: the
 * dispatch rule of the build (csrc/cc_gemm_plan.hpp), evaluated with the
 * default knobs whatever the environment says.  Host-only, touches no
 * device.  Validates like the GEMM entry points (same codes and
 * cc_last_error text); ldr is ignored when has_residual is 0. */
typedef struct cc_gemm_plan_info {
  int32_t body;       /* 128 or 256: block tile of the kernel body */
  int32_t tiles_x;    /* output tiles along N */
  int32_t tiles_y;    /* output tiles along M */
  int32_t grid;       /* workgroups launched (256² body: persistent fleet) */
  int32_t block;      /* threads per workgroup */
  int32_t xcd_remap;  /* 1 = tile order remapped for XCD L2 affinity */
  int32_t epi_staged; /* 1 = LDS-staged bf16 epilogue (256² body only) */
} cc_gemm_plan_info;
int cc_gemm_plan(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldr,
                 int has_bias, int act, int has_residual,
                 cc_gemm_plan_info* out);

/* ---- fused attention (ViT encoder; replaces torch sdpa + the qkv
 * permute copies).  qkv = the fused-QKV GEMM output [n*seq, 3*hidden]
 * bf16; out [n*seq, hidden] bf16; head dim hidden/heads = any multiple of 8
 * from 64 to 128 (64 CLIP/SigLIP-L, 72 SigLIP-so400m, 80 ViT-H, 88 ViT-g,
 * 104 bigG, ...); qkv and out 16-byte aligned.  cc_attn runs the rung of the ladder that cc::attn_plan
 * (csrc/cc_attn_plan.hpp) picks for seq — callers need not know the
 * thresholds:
 *   small  everything LDS-resident, one workgroup per (frame, head)
 *          (ViT-B/32's seq 50)
 *   mid    Q/K fragments straight from global, V^T + P in LDS, Q in 64-row
 *          tiles (ViT-L/14's 257, SigLIP-L16-256's 256)
 *   flash  K/V streamed in 64-row tiles with online softmax, one workgroup
 *          per (frame, head, q-tile) (SigLIP-384-class towers; above head
 *          dim 64 also most lengths from 65 to 288, e.g. so400m-224's 256)
 * CC_ERR_INVALID on null or misaligned pointers, non-positive
 * n_frames/seq/heads or a grid past 2^31-1 workgroups; CC_ERR_UNSUPPORTED
 * when hidden is not heads times such a head dim — all before any launch. */
int cc_attn(const void* qkv, void* out, int64_t n_frames, int seq, int heads,
            int hidden, float scale, uint64_t stream);

/* How a cc_attn call with these arguments would be launched.  Host-only,
 * touches no device.  Validates like cc_attn (same codes and cc_last_error
 * text), pointers aside. */
enum { CC_ATTN_SMALL = 0, CC_ATTN_MID = 1, CC_ATTN_FLASH = 2 };
typedef struct cc_attn_plan_info {
  int32_t rung;   /* CC_ATTN_SMALL | CC_ATTN_MID | CC_ATTN_FLASH */
  int32_t grid;   /* workgroups launched */
  int32_t block;  /* threads per workgroup */
} cc_attn_plan_info;
int cc_attn_plan(int64_t n_frames, int seq, int heads, int hidden,
                 cc_attn_plan_info* out);

/* One rung by name (kernel benches and the per-rung parity tests): cc_attn
 * restricted to that rung.  A seq the plan gives to another rung returns
 * CC_ERR_UNSUPPORTED. */
int cc_attn_small(const void* qkv, void* out, int64_t n_frames, int seq,
                  int heads, int hidden, float scale, uint64_t stream);
int cc_attn_mid(const void* qkv, void* out, int64_t n_frames, int seq,
                int heads, int hidden, float scale, uint64_t stream);
int cc_attn_flash(const void* qkv, void* out, int64_t n_frames, int seq,
                  int heads, int hidden, float scale, uint64_t stream);
/* A/B entry (tools/attn_hd_bench.py): run rung `rung` (CC_ATTN_*) wherever
 * it can cover seq, whatever the plan would pick — small seq <= 64, mid
 * seq <= 288, flash any.  CC_ERR_INVALID on an unknown rung,
 * CC_ERR_UNSUPPORTED on a seq the rung cannot cover. */
int cc_attn_rung(int rung, const void* qkv, void* out, int64_t n_frames,
                 int seq, int heads, int hidden, float scale, uint64_t stream);

/* CLS-query variant (head dim 64, any seq >= 1): attention for ONE query
 * row per (frame, head) against all seq keys/values — the only row of the
 * last encoder layer that hidden_states[:, 0] pooling reads (replaces the
 * last layer's torch sdpa under models/clip.py:71).  q [n_frames, hidden]
 * bf16; k and v point at the first key / value row of a buffer whose
 * rows (n_frames*seq of them) are ldkv elements apart, e.g. the two
 * halves of the K/V GEMM output [n_frames*seq, 2*hidden]; out
 * [n_frames, hidden] bf16.  ldkv >= hidden, ldkv % 8 == 0, pointers
 * 16-byte aligned. */
int cc_attn_cls(const void* q, const void* k, const void* v, int64_t ldkv,
                void* out, int64_t n_frames, int seq, int heads, int hidden,
                float scale, uint64_t stream);

/* ---- fused bf16 LayerNorm (replaces torch layer_norm in the ViT
 * forward; f32 stats/affine; H = 128, 1152, 1408 or one of the
 * instantiated multiples of 256: 256, 512, 768, 1024, 2048, 3072, 4096). */
int cc_layernorm_bf16(const void* x, const void* w, const void* b, void* y,
                      int64_t M, int64_t H, float eps, uint64_t stream);

/* ---- bf16 RMSNorm (InternVideo2), H as for
 * cc_layernorm_bf16, w f32 [H]:
 *   y = bf16( bf16(x * rsqrt(sum x^2 / H + eps)) * w )
 * f32 statistics; the normalised value is rounded to bf16 before the weight
 * multiply, the order of the model's own module.  Timed as "rmsnorm_bf16".
 * cc_qk_rmsnorm_bf16: the same, in place, on the q and k sections of a QKV
 * GEMM output qkv [M, ld] bf16: columns [0, H) of every row with wq,
 * columns [H, 2H) with wk, each section a norm of width H of its own;
 * columns from 2H on are not touched.  ld = row stride in elements, >= 2H,
 * ld % 4 == 0; one wave per (row, section).  Timed as "qk_rmsnorm".
 * Both: CC_ERR_INVALID on null pointers, non-positive sizes or a bad ld,
 * CC_ERR_UNSUPPORTED on another width, before any launch. */
int cc_rmsnorm_bf16(const void* x, const void* w, void* y, int64_t M,
                    int64_t H, float eps, uint64_t stream);
int cc_qk_rmsnorm_bf16(void* qkv, int64_t M, int64_t H, int64_t ld,
                       const void* wq, const void* wk, float eps,
                       uint64_t stream);

/* ---- LayerNorm folded into the GEMM that consumes it.
 * With W' = W * gamma (per column k, rounded to bf16), s[n] = sum_k W'[n,k]
 * (f32, of the rounded values) and c = W beta + b:
 *   act(linear(layer_norm(x), W, b)) = act(rstd*(W' x - mean*s) + c)
 * so the consuming GEMM reads the raw x and only needs (mean, rstd) per
 * row.  Row statistics travel as f32 partial sums per 64-column block,
 * stats [M, H/64, 2] = (sum x, sum x^2); no atomics, fixed summation
 * order, bit-identical from run to run.  H as for cc_layernorm_bf16.
 *
 * cc_ln_stats_bf16: the partials of x [M, H] bf16, one read-only pass
 * (timed as "ln_stats").
 * cc_ln_finalize: murstd[r] = (mean, rstd) [M, 2] f32 from the partials of
 * stats row r*row_step; var = sum x^2/H - mean^2, rstd = rsqrt(var + eps),
 * cc_layernorm_bf16's form (timed as "ln_finalize").
 * cc_gemm_bf16_res_stats: cc_gemm_bf16_ex(A, B, C, ..., bias, bf16 out,
 * act 0, residual) — C bit-identical to it — that also writes the
 * partials of the C rows it stores, stats [M, N/64, 2].  bias and residual
 * required.  The 256-tile body takes them in its epilogue; where the plan
 * picks the 128-tile body the entry runs the stats kernel on C afterwards.
 * cc_gemm_bf16_ln: C [M,N] bf16 = act(rstd*(A Wfold^T - mean*colsum) +
 * cbias).  A row i starts at A + i*row_step*K and its statistics are stats
 * row i*row_step (row_step 1 = dense; > 1 reads e.g. the CLS rows of a
 * [frames*seq, K] tensor in place, on the 128-tile body).  murstd is
 * [M, 2] f32 scratch the call fills (cc_ln_finalize) and reads.  Timed as
 * "gemm_bf16" plus "ln_finalize".
 * cc_rms_finalize / cc_gemm_bf16_rms: the RMSNorm forms.  RMSNorm is the
 * same expression with mean = 0 and rstd = rsqrt(sum x^2/H + eps), so
 * cc_rms_finalize writes murstd[r] = (0, rstd) from the same partials and
 * cc_gemm_bf16_rms is cc_gemm_bf16_ln running that finalize: with
 * Wfold = bf16(W * w_rms) per column and cbias = b (zeros for a layer
 * without bias), C = act(linear(rmsnorm(x))).  colsum is multiplied by the
 * zero mean; pass zeros.
 * All: CC_ERR_INVALID on null pointers or non-positive sizes,
 * CC_ERR_UNSUPPORTED on a width without LayerNorm kernels, before any
 * launch. */
int cc_ln_stats_bf16(const void* x, int64_t M, int64_t H, void* stats,
                     uint64_t stream);
int cc_ln_finalize(const void* stats, int64_t M, int64_t H, int64_t row_step,
                   float eps, void* murstd, uint64_t stream);
int cc_gemm_bf16_res_stats(const void* A, const void* B, void* C, int64_t M,
                           int64_t N, int64_t K, const float* bias,
                           const void* residual, void* stats, uint64_t stream);
int cc_gemm_bf16_ln(const void* A, int64_t row_step, const void* stats,
                    void* murstd, const void* Wfold, const float* colsum,
                    const float* cbias, void* C, int64_t M, int64_t N,
                    int64_t K, int act, float eps, uint64_t stream);
int cc_rms_finalize(const void* stats, int64_t M, int64_t H, int64_t row_step,
                    float eps, void* murstd, uint64_t stream);
int cc_gemm_bf16_rms(const void* A, int64_t row_step, const void* stats,
                     void* murstd, const void* Wfold, const float* colsum,
                     const float* cbias, void* C, int64_t M, int64_t N,
                     int64_t K, int act, float eps, uint64_t stream);

/* ---- fused ViT embedding assembly: out[f*tokens + t] =
 * LayerNorm( (t==0 ? cls : tok[f*(tokens-1)+t-1]) + pos[t] ).
 * Replaces the HF CLIPVisionEmbeddings cat + position-embedding add +
 * pre_layrnorm chain (reference models/clip.py get_image_features
 * entry).  tok bf16 [n_frames*(tokens-1), H]; cls/pos/w/b f32; out bf16
 * [n_frames*tokens, H]; H multiple of 256. */
int cc_embed_assemble_ln(const void* tok, const void* cls, const void* pos,
                         const void* w, const void* b, void* y,
                         int64_t n_frames, int64_t tokens, int64_t H,
                         float eps, uint64_t stream);

/* ---- TransNetV2 trunk: bf16 (2+1)D convolutions (csrc/cc_conv.hip) ----
 * Replace the f32 nn.Conv3d pairs of the shot detector's DDCNN blocks
 * (models/transnetv2.py:279-347, :224-277, :152-222).  Activations are bf16
 * channels-last [frames, H, W, C], accumulation is f32 in a fixed order with
 * no atomics: bit-identical from run to run and for any batch.  All
 * pointers 16-byte aligned (the u8 input aside).  Every entry checks its
 * arguments on the host before any launch, so a rejected call touches no
 * device: CC_ERR_INVALID on null or misaligned pointers and non-positive
 * sizes, CC_ERR_UNSUPPORTED on a channel count outside the stated set or a
 * grid past 2^31-1 workgroups.
 *
 * cc_conv3x3_bf16: y[n,h,w,co] = sum_{dy,dx,ci} x[n,h+dy,w+dx,ci] *
 * w[co,dy,dx,ci], zero padding 1, no bias, no activation.  x [frames,H,W,
 * Cin], w [Cout][3][3][Cin], y [frames,H,W,Cout]; Cin 64, 128 or 256, Cout a
 * multiple of 16 up to 512 (the four dilation branches of a block share
 * their input, so one launch computes all of them: Cout = 8F).  Implicit
 * GEMM on the 16x16x32 bf16 MFMA over the flattened (frame, pixel) index.
 * cc_conv3x3_u8: the same conv for the 3-channel first layer: x u8
 * [frames,H,W,3] taken as bf16(x/255) (f32 division, one rounding), w bf16
 * [Cout][3][3][3].  A plain FMA kernel (K = 27).  Both timed as "conv3x3".
 *
 * cc_tconv3_bf16: the four dilated 3-tap temporal convs of a block with its
 * folded BatchNorm.  x [B,T,HW,8F], w [4][F][3][2F], bias f32 [4F],
 * y [B,T,HW,4F]; branch b reads channels [b*2F, (b+1)*2F) at frames t-2^b,
 * t, t+2^b of the same window (zero padding at each window's ends, never
 * across windows) and writes channels [b*F, (b+1)*F):
 *   y = bf16(relu(acc + bias) + shortcut)
 * shortcut bf16 [B,T,HW,4F] or NULL (the stack tail relu(x) + shortcut).
 * F 16, 32 or 64; T >= 1.  Timed as "tconv3".
 *
 * cc_avgpool2x2_bf16: AvgPool3d((1,2,2)): [frames,H,W,C] -> [frames,H/2,
 * W/2,C], odd sizes floored, f32 sum and one rounding; C % 8 == 0, H and W
 * at least 2.  Timed as "avgpool". */
int cc_conv3x3_bf16(const void* x, const void* w, void* y, int64_t frames,
                    int H, int W, int Cin, int Cout, uint64_t stream);
int cc_conv3x3_u8(const void* x, const void* w, void* y, int64_t frames, int H,
                  int W, int Cout, uint64_t stream);
int cc_tconv3_bf16(const void* x, const void* w, const float* bias,
                   const void* shortcut, void* y, int64_t B, int T, int HW,
                   int F, uint64_t stream);
int cc_avgpool2x2_bf16(const void* x, void* y, int64_t frames, int H, int W,
                       int C, uint64_t stream);

/* ---- TransNetV2 heads (csrc/cc_tnheads.hip) ----------------------------
 * Everything after the trunk (models/transnetv2.py: ColorHistograms,
 * FrameSimilarity, fc1, cls_layer1), for all windows of a forward in one
 * pass.  Every sum is f32 in an order fixed by one window's shape: no float
 * atomics, no split-K, no workgroup across two windows, so results are
 * bit-identical from run to run and for any B, and a window never reads
 * another window's frames.  Any T >= 1.  Every entry checks its arguments on
 * the host before any launch, so a rejected call touches no device:
 * CC_ERR_INVALID on null or misaligned pointers (16 bytes; the u8 frames and
 * the f32 probabilities aside) and non-positive sizes, CC_ERR_UNSUPPORTED on
 * sizes outside the stated set.
 *
 * cc_tn_hist512_u8: frames_u8 [frames, pixels, 3] -> out f32 [frames, 512].
 * bin = (r>>5)<<6 | (g>>5)<<3 | (b>>5); integer counts c (LDS integer
 * atomics: order-free, exact); out = float(c) / fmaxf(sqrtf(float(sum c^2)),
 * 1e-12f).  pixels <= 4096 keeps sum c^2 <= 2^24 exact in f32, and with
 * correctly rounded sqrtf and division the result is bit-equal to the numpy
 * restatement.  One workgroup per frame.  Timed as "tn_hist512".
 *
 * cc_tn_framesim_embed: n_maps (1..3) pooled stack outputs x_i bf16
 * channels-last [frames, hw_i, c_i] -> out f32 [frames, 128].  Per frame the
 * spatial mean of every channel (f32 sum in ascending pixel order, then
 * / hw_i), the means concatenated in map order (c_i % 8 == 0, sum c_i <=
 * 512), then e[o] = chain over k ascending of fmaf(mean[k], proj_wt[k][o]) + proj_b[o]
 * with proj_wt f32 [sum c_i][128] (the Linear's weight transposed), then
 * out = e / fmaxf(sqrtf(sum e^2), 1e-12f).  out_dim must be 128.  One
 * workgroup per frame.  Timed as "tn_framesim_embed".
 *
 * cc_tn_simband_fc: x f32 [B, T, D], D 128 or 512.  s[j] = <x[b,t],
 * x[b,t+j-50]> for j = 0..100, 0 where the partner lies outside [0, T);
 * y[o] = relu(fc_b[o] + chain over j ascending of fmaf(fc_wt[j][o], s[j]))
 * for the 128 outputs, fc_wt f32 [101][128] (the Linear's weight
 * transposed; staged in LDS).  Written to out f32 [B*T, ldo] at columns
 * [col, col+128).  Only the band is computed, never the T x T matrix.  A
 * workgroup takes two consecutive frames of one window.  Timed as
 * "tn_simband_fc".
 *
 * cc_tn_fc1_relu: y f32 [M, N] = relu(bias + [hd | feat] . w^T) with hd f32
 * [M, KH], feat bf16 [M, KF], w_hi and w_lo bf16 [N][KH+KF] (w_hi = bf16(w),
 * w_lo = bf16(w - float(w_hi))), bias f32 [N].  On the 16x16x32 bf16 MFMA
 * into one f32 accumulator in this order: feat.w_hi, feat.w_lo, hd_hi.w_hi,
 * hd_hi.w_lo, hd_lo.w_hi, with hd_hi = bf16(hd), hd_lo = bf16(hd -
 * float(hd_hi)) formed in registers.  KH % 32 == 0, KF % 32 == 0,
 * N % 16 == 0.  One tile shape (a wave owns 32 rows x 32 outputs) for every
 * M; fragments straight from global memory, row tails guarded.  Timed as
 * "tn_fc1_relu".
 *
 * cc_tn_cls_sigmoid: p[m] = 1 / (1 + expf(-(b + sum_n w[n] * y[m,n]))), y f32
 * [M, N], w f32 [N], p f32 [M]; one wave per row, lane l chains n = l, l+64,
 * ... ascending, then a fixed butterfly.  Timed as "tn_cls_sigmoid". */
int cc_tn_hist512_u8(const void* frames_u8, void* out, int64_t frames,
                     int pixels, uint64_t stream);
int cc_tn_framesim_embed(const void* x0, const void* x1, const void* x2,
                         int hw0, int hw1, int hw2, int c0, int c1, int c2,
                         int n_maps, const float* proj_wt, const float* proj_b,
                         void* out, int64_t frames, int out_dim,
                         uint64_t stream);
int cc_tn_simband_fc(const float* x, const float* fc_wt, const float* fc_b,
                     void* out, int64_t B, int T, int D, int ldo, int col,
                     uint64_t stream);
int cc_tn_fc1_relu(const float* hd, const void* feat, const void* w_hi,
                   const void* w_lo, const float* bias, void* y, int64_t M,
                   int KH, int KF, int N, uint64_t stream);
int cc_tn_cls_sigmoid(const float* y, const float* w, float b, void* p,
                      int64_t M, int N, uint64_t stream);

/* ---- semantic dedup -------------------------------------------------
 * Strict-upper-triangular max-cosine scan (SemDedupActor.dedup,
 * pipelines/video/dedup/dedup_actor.py:315-460): for each row j of the
 * L2-normalized f32 matrix e[m][d] (scan order), the max cosine to any
 * earlier row and its argmax.  Row 0 -> (0.0, 0).  d % 64 == 0. */
int cc_pairwise_max_earlier(const void* e_f32, int64_t m, int64_t d,
                            void* maxv_f32, void* argi_i32, uint64_t stream);

/* ---- kernel timing (bench.py roofline evidence) ---------------------
 * When enabled, every cc_* kernel launch is bracketed with hipEvents on
 * its launch stream; totals are accumulated per kernel name. */
int cc_timing_enable(int enable);
int cc_timing_reset(void);
/* Fetch totals for `kernel` (e.g. "gemm_bf16"): total device ms + count. */
int cc_timing_report(const char* kernel, double* total_ms, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* CC_HOTPATH_H */
