/*
 * frhip.h -- C ABI of libfrhip.so: the MI355X (gfx950) detect -> align -> embed -> match hot path.
 *
 * The reference crosses into native code only through ONNX Runtime inside
 * insightface's FaceAnalysis.get (/root/reference/infrenceServer.py:412-416,528) and
 * through NumPy/BLAS for the match loop (/root/reference/infrenceServer.py:530-552).
 * These entry points are what a binding for that path binds instead.  Conventions:
 *   - every function returns 0 on success or a negative FR_E_* code;
 *     fr_last_error_string() gives the thread-local message;
 *   - no allocation inside: every buffer is device memory owned by the caller
 *     (PyTorch-ROCm tensors in the Python host), passed as plain pointers + sizes;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     launches are asynchronous, nothing synchronises;
 *   - no global mutable state and no environment variables: the only process-wide state is an atomic
 *     per-device bit per kernel remembering that its dynamic-LDS limit has been raised there (idempotent).
 * Each declaration cites the reference behaviour it replaces.
 */
#ifndef FRHIP_H
#define FRHIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FR_OK 0
#define FR_E_INVALID (-1)   /* bad argument / unsupported shape */
#define FR_E_LAUNCH (-2)    /* HIP launch error */
#define FR_E_NODEVICE (-3)  /* no gfx950 device */

typedef void* fr_stream_t;

/* Version of THIS header's ABI: bumped whenever a signature or an argument struct changes shape (101: fr_conv_args gained
 * x2 / C2, fr_conv_f8_args y8_sub, fr_pnet23_split_f16 all_heads; 103: the fr_gallery_topk_* / fr_match_reduce_shards_topk
 * entries; 104: fr_pnet_level gained x1s / hs / ws / f16, the fr_pnet_pyramid_* entries;
 * 105: fr_frame_ref, fr_letterbox_u8, fr_detections_unscale, the fr_warp_affine_5pt*_refs entries;
 * 106: fr_gallery_match_view_f16 / _f8 with their _workspace functions, fr_gallery_update_rows_shadow).  The SCRFD detector's
 * entries (fr_det_conv_f16, fr_det_conv_weight_halves, fr_det_input_f16, fr_det_pool_f16, fr_det_upsample_add_f16, fr_scrfd_decode)
 * were ADDED under 106: no existing signature or struct changed shape, and a binding written against them finds a library
 * without them by the missing symbol.  The same holds for fr_dw_conv_f16 and fr_det_conv_act_f16 (depthwise layers and the
 * PReLU epilogue of the plan recogniser, mbf.py), added under 106 later, and for fr_unknown_assign_batch_f32,
 * fr_gallery_first_above_blocked_f32 and fr_enrol_batch_f32 / fr_enrol_batch_workspace (the counting and enrolment paths in
 * batches), added under 106 after those, and for fr_gallery_match_grouped_f32 / fr_gallery_topk_grouped_f32 with their
 * _workspace functions (the grouped view scan of mixed-company batches), and for fr_gallery_pairs_above_f16 /
 * fr_gallery_pairs_workspace (the gallery audit), and for fr_yuv420_to_bgr_u8 / fr_yuv420_to_bgr_refs_u8 (YUV 4:2:0 frame ingest),
 * and for fr_frame_activity_u8 / fr_frame_activity_refs_u8 (the activity gate in front of the engine pass),
 * and for fr_pnet23_coarse_f16 / fr_pnet23_coarse_workspace_bytes / fr_pnet_pyramid_p23_coarse (the P-Net's coarse pass),
 * and for fr_track_associate_f32 / fr_track_commit_f32 (face tracks: a face's embedding carried across a camera's frames),
 * and for fr_face_quality_f16 (face quality: which aligned faces are worth the embed net),
 * and for fr_track_resolve_quality_i32 (judging face tracks: embed, carry or reject per face, only fit rows enter the bank),
 * and for fr_track_fuse_f32 (track templates: a track's last K shots fused into one scan query),
 * and for fr_hud_draw_u8 / fr_hud_draw_refs_u8 (the device HUD: recognition results drawn into the frames),
 * and for fr_jpeg_workspace / fr_jpeg_encode_u8 / fr_jpeg_encode_refs_u8 (the device JPEG encoder behind the HUD draw),
 * and for fr_jpeg_decode_workspace / fr_jpeg_decode_refs_u8 / fr_jpeg_blank_bad_refs_u8 (the device JPEG decoder in front of the
 * engine pass),
 * and for fr_jpeg_decode_oriented_refs_u8 (the same decoder writing each frame as its EXIF orientation turns it),
 * and for fr_redact_u8 / fr_redact_refs_u8 (face redaction: regions pixelated or filled in place in front of the HUD draw),
 * and for fr_face_chips_u8 / fr_face_chips_refs_u8 (face chips: a square around each face cut and resampled to a thumbnail),
 * ADDED under 106 likewise.  fr_version() returns the value the library was built
 * with: a caller compiled against another header must refuse to go on (the Python binding does, _lib.load()). */
#define FR_ABI_VERSION 106
int fr_version(void);
const char* fr_last_error_string(void);
/* number of visible HIP devices (<=0: none); does not create a context on any device */
int fr_device_count(void);

/* ---------------------------------------------------------------- match ----
 * a-6  q = normed_embedding / ||normed_embedding||   (infrenceServer.py:532, peopleCount.py:863)
 * also the gallery-row normalise v/||v||              (infrenceServer.py:271,324) */
int fr_l2norm_rows_f32(const float* x, float* out, int rows, int dim, fr_stream_t stream);

/* a-7  best = -1; for id,g in gallery: s = dot(q,g); if s > best: best,id = s,id
 *      (infrenceServer.py:535-542, peopleCount.py:866-873).  Rows carry their index as id;
 *      strict '>' => the lowest row index wins exact ties.  Q [F,D] f32 (re-normalised),
 *      G [N,D] f32 row-major, D == 512.  out_idx[f] = row + row_offset (or -1 when N == 0),
 *      out_score[f] = best dot (or -1).  workspace: fr_gallery_match_workspace() bytes.
 *      seg_counts (optional, device i32 [F / seg_len]) marks padding: query slot f is real iff
 *      f % seg_len < seg_counts[f / seg_len] (the gathered per-rank face counts of the sharded match, 8(e));
 *      padding slots cost no scan work and report (-1, -1).  NULL: every slot is real. */
size_t fr_gallery_match_workspace(int F, int64_t N);
int fr_gallery_match_f32(const float* Q, const float* G, int F, int64_t N, int D,
                         int64_t row_offset, int64_t* out_idx, float* out_score,
                         void* workspace, size_t workspace_bytes, const int32_t* seg_counts, int seg_len,
                         fr_stream_t stream);
/* Gallery slab + views (replaces the per-frame dict filtering of
 * infrenceServer.py:343-380 and the dict inserts/deletes of :260-341, :234-258).  G is one device-resident
 * slab of row slots [capacity,512]; a view is the int64 slot list of one company in the reference's dict
 * order.  fr_gallery_match_view_f32 scans rows G[view[0..Nview)] without copying them; out_idx is the VIEW
 * position (so "first maximum in iteration order" is the view's order), -1 when Nview == 0.
 * fr_gallery_update_rows_f32 writes rows[i] (optionally v/||v||, :271,324) into slot slots[i] in place. */
int fr_gallery_match_view_f32(const float* Q, const float* G, const int64_t* view, int F, int64_t Nview, int D,
                              int64_t* out_idx, float* out_score, void* workspace, size_t workspace_bytes,
                              fr_stream_t stream);
int fr_gallery_update_rows_f32(float* G, const int64_t* slots, const float* rows, int n, int D, int normalise,
                               fr_stream_t stream);
/* Large galleries / many queries (BASELINE configs C4, C5): ONE pass over a 16-bit or 8-bit copy of the gallery
 * on the f16 / fp8 matrix cores for up to 256 queries per block keeps the top FR_TOPK (f16) / FR_TOPK8 (fp8)
 * rows per query, which are then re-scored EXACTLY in f32 against G32 (may be NULL: scores then come from the
 * coarse scan) and picked by max score / lowest row - the rule of infrenceServer.py:535-542.
 * G16: f16 [N,512] (fr_f32_to_f16 of the unit rows); G8: OCP fp8 e4m3 [N,512] scaled by FR_F8_SCALE
 * (fr_f32_to_f8).  seg_counts / seg_len: see fr_gallery_match_f32.
 * With G32 == NULL nothing is re-scored and the result is the coarse scan's own: out_score[f] is the coarse maximum -
 * the largest dot product of the stored operands (the f16 roundings of query and rows; fp8: the e4m3 codes of
 * 256 x query and 256 x row, saturated at +-448, the sum divided by 256^2), accumulated in f32 on the matrix cores -
 * and out_idx[f] is the first row of the first group of 4 consecutive rows (rows 4g .. 4g + 3) that attains it, plus
 * row_offset: a multiple of 4 plus row_offset, not necessarily the row that scored.  (-1, -1.0f) if no coarse score
 * exceeds -1.  The view forms have no such mode: they refuse a NULL G32. */
#define FR_TOPK 4
#define FR_TOPK8 8
#define FR_F8_SCALE 256.0f
size_t fr_gallery_match_f16_workspace(int F, int64_t N);
int fr_gallery_match_f16(const float* Q, const void* G16, const float* G32, int F, int64_t N, int D,
                         int64_t row_offset, int64_t* out_idx, float* out_score,
                         void* workspace, size_t workspace_bytes, const int32_t* seg_counts, int seg_len,
                         fr_stream_t stream);
size_t fr_gallery_match_f8_workspace(int F, int64_t N);
int fr_gallery_match_f8(const float* Q, const void* G8, const float* G32, int F, int64_t N, int D,
                        int64_t row_offset, int64_t* out_idx, float* out_score,
                        void* workspace, size_t workspace_bytes, const int32_t* seg_counts, int seg_len,
                        fr_stream_t stream);
/* a-7, K best: exact top-K identification.  The top-K list of a query is the first K rows under the total order
 * (score descending, row ascending) among rows whose score is > -1.0f - the rule of a-7 (best starts at -1, strict
 * '>', first maximum) extended from 1 to K; rows are counted in scan order (view position for a view).  Slots past
 * the number of such rows hold (idx -1, score -1.0f), as does every slot of a padding query and of a NaN query.
 * Scores are the same f32 dot products, in the same summation order, as fr_gallery_match_f32 computes, so column 0
 * (out_idx[f][0], out_score[f][0]) is bit-identical to fr_gallery_match_f32 / _view_f32 for every K.
 * 1 <= K <= FR_TOPK_MAX.  out_idx / out_score: [F][K]; filled slots carry row + row_offset.  workspace:
 * fr_gallery_topk_workspace() bytes, holding the per-block partial lists [blocks][F][K] (f32 scores, then int64 rows).
 * F == 0 returns FR_OK without reading a pointer; N == 0 writes (-1, -1.0f) everywhere.
 * seg_counts / seg_len: see fr_gallery_match_f32. */
#define FR_TOPK_MAX 16
size_t fr_gallery_topk_workspace(int F, int64_t N, int K);
int fr_gallery_topk_f32(const float* Q, const float* G, int F, int64_t N, int D, int K, int64_t row_offset,
                        int64_t* out_idx /*[F][K]*/, float* out_score /*[F][K]*/, void* workspace,
                        size_t workspace_bytes, const int32_t* seg_counts, int seg_len, fr_stream_t stream);
int fr_gallery_topk_view_f32(const float* Q, const float* G, const int64_t* view, int F, int64_t Nview, int D,
                             int K, int64_t* out_idx, float* out_score, void* workspace,
                             size_t workspace_bytes, fr_stream_t stream);
/* The coarse scan through a view: a deployment's synced slab at the sizes above.  S16 / S8 is a second slab
 * [capacity,512] beside the f32 slab G32, f16 or OCP fp8 e4m3 x FR_F8_SCALE, whose slot s holds exactly
 * fr_f32_to_f16 / fr_f32_to_f8 of G32's slot s; fr_gallery_update_rows_shadow keeps it so by writing both slabs in
 * ONE launch (shadow_kind FR_SHADOW_F16 / FR_SHADOW_F8; otherwise fr_gallery_update_rows_f32's contract).  Slots no
 * view names may hold anything.
 * fr_gallery_match_view_f16 / _f8 scan the coarse rows S[view[0..Nview)] on the matrix cores, keep the FR_TOPK /
 * FR_TOPK8 best groups of 4 consecutive VIEW positions per query and re-score those exactly in f32 against
 * G32[view[pos]].  The result contract is fr_gallery_match_view_f32's: out_idx is the VIEW position of the maximum f32
 * score, the lowest position on exact ties, (-1, -1.0f) when Nview == 0 or no score exceeds -1; out_score is the f32
 * dot.  workspace: the matching _workspace(F, Nview) bytes.
 * Limits: Nview < 2^31 and capacity < 2^31 slots; every view[i] must lie in [0, capacity) (slot numbers are read as
 * 32-bit values, and nothing checks them).  Each row is fetched through a 64-bit address, so the slab's BYTE size is
 * not limited: a 4 M-slot f16 slab (4 GiB) or a 10 M-slot fp8 slab (5 GiB) is addressed exactly.  A capacity or Nview
 * past the limit is refused with FR_E_INVALID, never wrapped. */
#define FR_SHADOW_F16 1
#define FR_SHADOW_F8 2
int fr_gallery_update_rows_shadow(float* G, void* shadow, int shadow_kind, const int64_t* slots, const float* rows,
                                  int n, int D, int normalise, fr_stream_t stream);
size_t fr_gallery_match_view_f16_workspace(int F, int64_t Nview);
int fr_gallery_match_view_f16(const float* Q, const void* S16, const float* G32, const int64_t* view, int F,
                              int64_t Nview, int64_t capacity, int D, int64_t* out_idx, float* out_score,
                              void* workspace, size_t workspace_bytes, fr_stream_t stream);
size_t fr_gallery_match_view_f8_workspace(int F, int64_t Nview);
int fr_gallery_match_view_f8(const float* Q, const void* S8, const float* G32, const int64_t* view, int F,
                             int64_t Nview, int64_t capacity, int D, int64_t* out_idx, float* out_score,
                             void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* Certified coarse top-K: fr_gallery_topk_f32 / _view_f32's result, bit for bit, from ONE pass over the f16 rows on the
 * matrix cores wherever that pass provably suffices, from the exact scan for every other query - decided per query on
 * the device.  The coarse pass keeps, per query, candidate groups of 4 consecutive rows and a bound on the coarse score
 * of every row it did not keep; the re-rank re-scores the rows of the best groups with the exact scan's own f32 dot
 * product (same bits), and certifies a query iff its K-th exact score exceeds every unseen row's coarse bound by more
 * than eps = 1.125 * 2^-10 * |q| * Gmax + 2^-20 * (|q| + Gmax) + 2^-40, a proven bound of |coarse - exact| (DESIGN.md
 * 4.6b).  flags (device int32 [F]): 0 = certified, 1 = answered by the exact scan (also: any query with a non-finite
 * element or one beyond the f16 range).  Queries that are flagged cost an exact scan; when none is, the exact launch
 * finds no work.
 * gmax: device float [1], an upper bound of the largest row norm in G32 / the slab; fr_gallery_gmax_update raises it
 * to cover rows G[slots[0..n)] (slots NULL: rows 0..n) and sets it to +inf when a row holds a non-finite element or
 * one that overflows f16 (|x| > 65504) - then nothing certifies.  It never shrinks: start it at 0, call the update on
 * the stream that wrote the rows.
 * Contract, arguments and limits otherwise as fr_gallery_topk_f32 / fr_gallery_topk_view_f32 and
 * fr_gallery_match_f16 / _view_f16 (G16 / S16: fr_f32_to_f16 of the f32 rows), and N <= 2^28 rows.
 * fr_gallery_topk_view_masked_f32: fr_gallery_topk_view_f32 for the queries f with mask[f] > 0 (device int32 [F]; NULL:
 * all); the others cost no scan work and report (-1, -1.0f). */
size_t fr_gallery_topk_f16_workspace(int F, int64_t N, int K);
int fr_gallery_topk_f16(const float* Q, const void* G16, const float* G32, int F, int64_t N, int D, int K,
                        int64_t row_offset, const float* gmax, int64_t* out_idx, float* out_score, int32_t* flags,
                        void* workspace, size_t workspace_bytes, const int32_t* seg_counts, int seg_len,
                        fr_stream_t stream);
size_t fr_gallery_topk_view_f16_workspace(int F, int64_t Nview, int K);
int fr_gallery_topk_view_f16(const float* Q, const void* S16, const float* G32, const int64_t* view, int F,
                             int64_t Nview, int64_t capacity, int D, int K, const float* gmax, int64_t* out_idx,
                             float* out_score, int32_t* flags, void* workspace, size_t workspace_bytes,
                             fr_stream_t stream);
int fr_gallery_topk_view_masked_f32(const float* Q, const float* G, const int64_t* view, int F, int64_t Nview, int D,
                                    int K, int64_t* out_idx, float* out_score, void* workspace,
                                    size_t workspace_bytes, const int32_t* mask, fr_stream_t stream);
int fr_gallery_gmax_update(const float* G, const int64_t* slots, int64_t n, int D, float* gmax, fr_stream_t stream);
/* Grouped view scan: every query through ITS OWN view of the slab G [capacity,512], in one launch pair - a batch whose
 * frames belong to different companies.  The exact f32 scan only: on a slab that also keeps a coarse copy these
 * entries still read G.
 *   Q       f32 [F][512]: ALL query slots in slot order, neither permuted nor compacted.
 *   views   int64 [V]: the slot lists of the distinct views, concatenated (V >= 1 elements allocated).
 *   gtab    int64 [ngroups][2]: per query group (offset into views, view length).  Several groups may name one view.
 *   qmap    int32 [ngroups * 32]: the query slot that lane r of group g owns (entry g * 32 + r), or -1.  A slot should
 *           appear in at most one entry.
 *   max_view_len: the longest view length in gtab; it sizes the grid and the workspace only - the rows of a longer
 *           view are still all scanned (the tile loop strides over the grid).
 *   capacity: slots of G, < 2^31 (refused with FR_E_INVALID beyond, as the coarse view entries refuse it).  Every
 *           views[] entry must lie in [0, capacity); they, and the offsets and lengths in gtab, are read as given and
 *           not checked, as fr_gallery_match_view_f32 reads its view.
 *   seg_counts / seg_len: see fr_gallery_match_f32 (they speak of query SLOTS, f = position in Q).
 * Result, for every query slot f that some qmap entry names: out_idx[f] = the POSITION IN f's VIEW (not the slab slot)
 * of the maximum score, lowest position on exact ties, and out_score[f] - bit for bit what fr_gallery_match_view_f32
 * returns for query f alone against that view (the same k-ordered f32 chains - measured to be the fmaf chain over
 * elements 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, ..., docs/KERNEL_NOTES.md 4.15; neither group nor lane matters);
 * (-1, -1.0f) for a padding slot, an empty view, or when no score exceeds -1.  fr_gallery_topk_grouped_f32: the same for
 * fr_gallery_topk_view_f32, out_idx / out_score [F][K].  QUERY SLOTS THAT NO qmap ENTRY NAMES ARE NOT WRITTEN.
 * A group whose view is empty or whose slots are all padding costs no scan work.  ngroups <= 65535.  F == 0 or
 * ngroups == 0 returns FR_OK without a launch.  workspace: the matching _workspace(ngroups, max_view_len[, K]) bytes
 * (partial results [blocks][ngroups * 32]). */
size_t fr_gallery_match_grouped_workspace(int ngroups, int64_t max_view_len);
int fr_gallery_match_grouped_f32(const float* Q, const float* G, const int64_t* views, const int64_t* gtab,
                                 const int32_t* qmap, int F, int ngroups, int64_t max_view_len, int64_t capacity, int D,
                                 int64_t* out_idx, float* out_score, void* workspace, size_t workspace_bytes,
                                 const int32_t* seg_counts, int seg_len, fr_stream_t stream);
size_t fr_gallery_topk_grouped_workspace(int ngroups, int64_t max_view_len, int K);
int fr_gallery_topk_grouped_f32(const float* Q, const float* G, const int64_t* views, const int64_t* gtab,
                                const int32_t* qmap, int F, int ngroups, int64_t max_view_len, int64_t capacity, int D,
                                int K, int64_t* out_idx /*[F][K]*/, float* out_score /*[F][K]*/, void* workspace,
                                size_t workspace_bytes, const int32_t* seg_counts, int seg_len, fr_stream_t stream);
/* f32 -> fp8 e4m3 row conversion (x * FR_F8_SCALE, round to nearest even, n % 4 == 0) */
int fr_f32_to_f8(const float* x, void* out, int64_t n, fr_stream_t stream);
/* f32 -> f16 row conversion for building the device-resident gallery (infrenceServer.py:271) */
int fr_f32_to_f16(const float* x, void* out, int64_t n, fr_stream_t stream);
/* a-8  known = best_id and best >= thr  (infrenceServer.py:545; peopleCount.py:876-882):
 *      decision[f] = 1 recognised, 0 unknown, 2 dropped (counting path's [unknown_thr, thr) band;
 *      pass unknown_thr = thr for the live path). */
int fr_match_decide(const int64_t* idx, const float* score, int F, float thr, float unknown_thr,
                    int32_t* decision, fr_stream_t stream);


/* e   Sharded match (the reference's only parallelism is one process per camera, each scanning
 *      the whole gallery: infrenceServer.py:606,641-646).  Every rank scans ITS gallery row shard for all gathered
 *      queries (fr_gallery_match_* with row_offset = the shard's first global row); candidates travel as
 *      int32 [n][3] = (score bits, row lo, row hi) so the all-gather moves raw bits; the reduce over the R shards
 *      for queries [q0, q0+F) applies the scan's own rule - maximum score, lowest global row on exact ties,
 *      (-1, -1.0) when no shard has a candidate (infrenceServer.py:535-542).  cand_all: int32 [R][n][3]. */
int fr_match_pack_candidates(const int64_t* idx, const float* score, int n, int32_t* cand, fr_stream_t stream);
int fr_match_reduce_shards(const int32_t* cand_all, int R, int n, int q0, int F, int64_t* out_idx,
                           float* out_score, fr_stream_t stream);
/*      Top-K form: every shard contributes its K best per query slot (fr_gallery_topk_f32 with row_offset);
 *      fr_match_pack_candidates packs the flat n*K list unchanged, so cand_all is int32 [R][n][K][3].  The reduce
 *      writes, for queries [q0, q0+F), the K best of the R lists under the same total order (score descending, global
 *      row ascending) to out_idx / out_score [F][K]; a row < 0 is an empty slot, empty output slots are (-1, -1.0). */
int fr_match_reduce_shards_topk(const int32_t* cand_all, int R, int n, int K, int q0, int F,
                                int64_t* out_idx, float* out_score, fr_stream_t stream);
/*      Exchange buffers of the same step: send f32 [q_max+1][D] = the rank's F unit query rows, zero rows up to q_max,
 *      and one trailing row whose first element is F (the face count rides in the one all-gather); after the gather
 *      (f32 [R][q_max+1][D]) counts[r] = that element of rank r's block.  The scan then walks the gathered buffer in
 *      place with seg_len = q_max + 1: the count row is slot q_max >= count, i.e. padding. */
int fr_exchange_pack_queries(const float* Q, int F, int q_max, int D, float* send, fr_stream_t stream);
int fr_exchange_counts(const float* gathered, int R, int q_max, int D, int32_t* counts, fr_stream_t stream);


/* ------------------------------------------------- enrolment / clustering consumers of the scan ----
 * First (lowest) row whose dot with the query is > thr (inclusive != 0: >= thr); idx -1 / score 0 when none.
 * Duplicate check `sim > 0.4`, first hit returns (trainingServer.py:181-194); unknown-person assignment
 * `similarity >= 0.65`, first hit breaks (peopleCount.py:441-449).  Rows must be unit length for the
 * dot to be the reference's cosine.  workspace: F * 8 bytes. */
int fr_gallery_first_above_f32(const float* Q, const float* G, int F, int64_t N, int D, float thr,
                               int inclusive, int64_t row_offset, int64_t* out_idx, float* out_score,
                               void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* out[f][n] = cosine(A[f], B[n]): pose-consistency matrix (trainingServer.py:202-214) */
int fr_cosine_matrix_f32(const float* A, const float* B, int F, int N, int D, float* out,
                         fr_stream_t stream);
/* out = mean of K rows, summed in row order (np.mean(.., axis=0): trainingServer.py:355, peopleCount.py:79) */
int fr_mean_rows_f32(const float* x, int K, int D, float* out, fr_stream_t stream);
/* Unknown-person clustering of a whole batch in ONE launch (peopleCount.py:441-449 + UnknownPerson.update :68-75), the
 * rows of E [F][512] in order, row f taken when take == NULL or take[f] != 0:
 *   hit  = lowest c < n with dot(avg[c], E[f]) >= thr (f32, inclusive; the dot of fr_gallery_first_above_f32, same bits):
 *          E[f] is pushed into cluster c's ring (depth rows, the oldest is overwritten once full), its detection_count
 *          goes up by one and avg[c] = (oldest + ... + newest) / (float)K, summed in that order (np.mean of the deque);
 *   miss = cluster n is created: avg[n] = E[f] as is, ring = that one row, detection_count 1, n += 1;
 *   miss with n == capacity: nothing changes, out_cluster[f] = -2 and the sticky overflow counter goes up by one.
 * out_cluster[f]: the cluster index (-1: row not taken, -2: refused at capacity); out_new[f]: 1 when the row created its
 * cluster; out_count[f]: the cluster's detection_count after the row (0 for -1 / -2).
 * State, all caller-owned device memory that only this entry writes: avg f32 [capacity][512], hist f32 [capacity][depth][512],
 * state int32 [FR_UNKNOWN_STATE_INTS(capacity)] - zero it once to start empty: [FR_UNKNOWN_N] live clusters,
 * [FR_UNKNOWN_OVERFLOW] refused rows, then per cluster c at FR_UNKNOWN_HEADER + 3 c: ring length, ring head (the slot the
 * next push writes), detection_count.  One workgroup walks the batch (the row-to-row dependency is real); no allocation,
 * no synchronisation.  Added under ABI 106: no existing signature changed. */
#define FR_UNKNOWN_N 0
#define FR_UNKNOWN_OVERFLOW 1
#define FR_UNKNOWN_HEADER 4
#define FR_UNKNOWN_STATE_INTS(capacity) (FR_UNKNOWN_HEADER + 3 * (capacity))
int fr_unknown_assign_batch_f32(const float* E, const int32_t* take, int F, int D, float thr, float* avg, float* hist,
                                int32_t* state, int capacity, int depth, int32_t* out_cluster, int32_t* out_new,
                                int32_t* out_count, fr_stream_t stream);

/* fr_gallery_first_above_f32 for MANY queries: the same result contract (out_idx[f] = the first position whose dot with
 * Q[f] passes the threshold, + row_offset; -1 / 0.f when none) and, for every (query, gallery) pair the older entry can
 * express, the same index and the same score bits.  What differs is the traffic: a gallery row is fetched once per block of
 * 16 queries, not once per query.
 *   view == NULL: position p is row p of G [N][512].  view != NULL: position p is row view[p] of G (int64 storage slots of a
 *   slab, read as given and not checked, as fr_gallery_match_view_f32 reads them); out_idx is the VIEW position.
 *   take == NULL: every query is scanned.  take != NULL (int32 [F]): query f with take[f] == 0 costs no scan work and
 *   reports -1 / 0.f.
 * N < 2^31.  workspace: F * 8 bytes.  Added under ABI 106. */
int fr_gallery_first_above_blocked_f32(const float* Q, const float* G, const int64_t* view, const int32_t* take, int F,
                                       int64_t N, int D, float thr, int inclusive, int64_t row_offset, int64_t* out_idx,
                                       float* out_score, void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* Enrolment of J jobs in one call (trainingServer.py:170-247, 312-398 for a whole batch): job for job the result of
 * enrolling the jobs one after the other, every `done` job's row being visible to the duplicate check of the later jobs.
 * Inputs, all on the device: E f32 [S][512] normed embeddings and bbox f32 [S][4] (x1, y1, x2, y2), one row per face slot;
 * image i owns rows img_first[i] .. img_first[i] + img_count[i] - 1 (img_count: the face counts as the detector wrote
 * them; both are clamped so that no row outside [0, S) is read); job j owns images job_first[j] .. job_first[j+1] - 1 of
 * the I images, in the caller's order (job_first int32 [J+1]).  max_poses: the largest number of images of a job, which
 * the caller knows on the host.  The gallery: G / view / N as fr_gallery_first_above_blocked_f32, unit rows.
 * Per job, in job order:
 *   1. per image, the face = the first slot with the largest area (x2 - x1) * (y2 - y1), f32, each operation rounded
 *      once, strict '>' in slot order; an image with no face is skipped.  face[i] = that slot, -1 for no face.
 *   2. K faces found; K == 0: FR_ENROL_NO_FACE.
 *   3. pairs (a, b), a < b, in lexicographic order over the K found embeddings: the first with cosine < sim_thr (the bits
 *      of fr_cosine_matrix_f32) -> FR_ENROL_DIFFERENT, pair[j] = (a, b) (indices among the FOUND embeddings).
 *   4. avg[j] = the K rows summed in order / (float)K (the bits of fr_mean_rows_f32); not re-normalised.
 *   5. q = avg / ||avg|| (the bits of fr_l2norm_rows_f32, which are the bits fr_gallery_update_rows_f32(normalise=1) stores:
 *      row[j] is both the job's query and the row it enrols).  The first gallery position p with dot(q, row_p) > dup_thr
 *      (fr_gallery_first_above_f32's dot and bits) -> FR_ENROL_DUPLICATE, dup_pos[j] = p, dup_score[j] = that dot.
 *   6. otherwise the first earlier job i < j that ended FR_ENROL_DONE with dot(q, row[i]) > dup_thr -> FR_ENROL_DUPLICATE,
 *      dup_pos[j] = N + i.  A gallery hit always wins (gallery rows come first); jobs that did not end DONE add no row.
 *   7. otherwise FR_ENROL_DONE.
 * Outputs, device: status int32 [J]; pair int32 [J][2] ((-1, -1) unless DIFFERENT); face int32 [I]; avg f32 [J][512]
 * (zero rows for NO_FACE / DIFFERENT); row f32 [J][512] (the unit row of a DONE / DUPLICATE job, else zero); dup_pos
 * int64 [J] (-1 unless DUPLICATE); dup_score f32 [J] (0 unless DUPLICATE).
 * Four launches whatever J, I and N are, no allocation, no synchronisation.  J > FR_ENROL_MAX_JOBS, max_poses >
 * FR_ENROL_MAX_POSES and D != 512 are refused before any launch; J == 0 returns FR_OK and reads no pointer.
 * workspace: fr_enrol_batch_workspace(J, N) bytes.  Added under ABI 106. */
#define FR_ENROL_DONE 0
#define FR_ENROL_NO_FACE 1
#define FR_ENROL_DIFFERENT 2
#define FR_ENROL_DUPLICATE 3
#define FR_ENROL_MAX_POSES 8
#define FR_ENROL_MAX_JOBS 256
size_t fr_enrol_batch_workspace(int J, int64_t N);
int fr_enrol_batch_f32(const float* E, const float* bbox, int S, const int32_t* img_first, const int32_t* img_count, int I,
                       const int32_t* job_first, int J, int max_poses, int D, const float* G, const int64_t* view, int64_t N,
                       float sim_thr, float dup_thr, int32_t* status, int32_t* pair, int32_t* face, float* avg, float* row,
                       int64_t* dup_pos, float* dup_score, void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* Gallery audit: ALL pairs of positions 0 <= a < b < N of a view (position p = row G32[view[p]]; view NULL: row p) with
 *   s(a, b) = the dot of fr_gallery_first_above_f32 of the two rows as stored (not renormalised, the same bits; symmetric)
 *   s > thr  (inclusive: s >= thr), in f32
 * - the pairs the enrolment duplicate check would refuse.  EXACT for every view whose rows are finite and inside the f16
 * range: an f16 matrix-core pass over the pairs only filters (coarse score >= thr - eps, eps = 1.125 2^-10 Gmax^2 +
 * 2^-20 2 Gmax + 2^-40 with Gmax the largest row norm of the view: DESIGN.md 4.6f), every candidate is re-scored with
 * that dot and kept or dropped by it alone.  The coarse slab of a scan="f16" / "f8" gallery is not read.
 * out_key int64 [capacity]: a << 32 | b; out_score f32 [capacity]: s beside it; both UNORDERED, out_counts[1] entries.
 * out_counts int32 [4]: [0] candidates the filter saw (it keeps counting past capacity), [1] pairs written, [2] flags,
 * [3] row ranges the plan used.  FR_PAIRS_OVERFLOW: more candidates than capacity - the pairs written are a subset of the
 * true set, retry with capacity >= out_counts[0].  FR_PAIRS_NONFINITE: a row of the view holds NaN, an infinity or an
 * element beyond +-65504 (what fr_gallery_gmax_update reports) - no pair is written.
 * max_ranges: 0, or an upper bound on the row ranges the scan is cut into (tuning).  N < 2^31, D == 512, 1 <= capacity <
 * 2^31; N <= 1: zero counts (out_counts may be NULL), no row is read.  workspace: fr_gallery_pairs_workspace(N, capacity)
 * bytes (Gmax, the candidates, the f16 copy of the view's rows).  Two memsets and four launches whatever N; no allocation,
 * no synchronisation.  Added under ABI 106. */
#define FR_PAIRS_OVERFLOW 1
#define FR_PAIRS_NONFINITE 2
size_t fr_gallery_pairs_workspace(int64_t N, int64_t capacity);
int fr_gallery_pairs_above_f16(const float* G32, const int64_t* view, int64_t N, int D, float thr, int inclusive,
                               int64_t capacity, int max_ranges, int64_t* out_key, float* out_score, int32_t* out_counts,
                               void* workspace, size_t workspace_bytes, fr_stream_t stream);

/* ---------------------------------------------------------------- embed ----
 * a-4  ArcFace IResNet conv stack (inside FaceAnalysis.get, infrenceServer.py:528).
 * Implicit-GEMM convolution on MFMA, NHWC f16 activations, f32 accumulate:
 *   y[n,ho,wo,co] = epi( sum_{kh,kw,ci} x[n,ho*s+kh-p,wo*s+kw-p,ci] * w[co,kh,kw,ci] )
 *   epi(v) = prelu(v + bias) (+ residual)
 * w: [Cout][KH*KW*Cin] f16 (K contiguous).  Cin % 64 == 0, or Cin == 8 (packed stem: w rows
 * zero-padded to a multiple of 128).  Cout % 64 == 0.
 * bias: f32 [Cout] (bias_mode 0) or [9][Cout] (bias_mode 1: border-class bias
 * [row class: top/mid/bottom][col class: left/mid/right] that carries a folded
 * pre-activation BN shift through the zero padding; 3x3/s1/p1 only), or NULL.
 * slope: f32 [Cout] PReLU slopes or NULL.  residual: f16 [M,Cout] or NULL.
 * out_f32_partial != NULL: split-K mode, raw f32 partial sums [splitk][M][Cout]
 * (no epilogue), used for the FC 25088->512 (H=W=1, Cin=25088).
 * x2 != NULL: a second input [B,H,W,C2] f16 (same H, W as x; C2 % 64 == 0) that enters through a 1x1 tap at
 * (ho * stride, wo * stride) as C2 extra K rows - w is then [Cout][KH*KW*Cin + C2].  An IResNet stage-entry block's
 * 1x1 / stride-2 shortcut conv of the block input, summed with its stride-2 3x3 conv in ONE implicit GEMM (f32
 * accumulation; biases summed by the caller) instead of a launch, an f16 map written and read back. */
typedef struct {
    const void* x; const void* w; void* y;
    const float* bias; const float* slope; const void* residual;
    float* out_f32_partial;
    int B, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo;
    int bias_mode; int splitk;
    const void* x2; int C2;
} fr_conv_args;
int fr_conv_nhwc_f16(const fr_conv_args* args, fr_stream_t stream);
/* fp8 form of the body convs (BASELINE config C5: "fp8 ArcFace conv path, CDNA4 fp8 MFMA"; same reference site,
 * infrenceServer.py:528): 3x3 / stride 1 / pad 1 layers at 14x14 and 28x28 (78 % of the r100 FLOPs) on
 * v_mfma_scale_f32_16x16x128_f8f6f4.  x8: OCP fp8 e4m3 NHWC [B,H,W,Cin] = x / sx; w8: e4m3 [Cout][9*Cin] =
 * w / sw[cout] (per-output-channel); oscale[cout] = sw[cout] * sx dequantises the f32 accumulator, then the f16
 * kernel's epilogue: + bias (or 9-class border bias) -> PReLU -> + residual (f16) -> one rounding.  Outputs:
 * y16 (f16 NHWC, may be NULL) and/or y8 = fp8((y - y8_sub[cout]) * y8_mul) (the next conv's input, may be NULL;
 * y8_sub: f32 [Cout] per-channel centre the CONSUMER subtracts from its input before rounding - its W.centre term,
 * which depends on which taps fall inside the image, lives in the consumer's 9-class border bias - or NULL = 0).
 * Cin % 128 == 0, Cout % 128 == 0. */
typedef struct {
    const void* x8; const void* w8; void* y16; void* y8;
    const float* oscale; const float* bias; const float* slope; const void* residual;
    int B, H, W, Cin, Cout, bias_mode;
    float y8_mul;
    const float* y8_sub;
} fr_conv_f8_args;
int fr_conv_nhwc_f8(const fr_conv_f8_args* args, fr_stream_t stream);
/* out8 = fp8_e4m3(x16 * mul), saturating at +-448; n % 8 == 0 (input of a stage's first fp8 conv) */
int fr_quantize_f16_f8(const void* x16, void* out8, int64_t n, float mul, fr_stream_t stream);
/* out8 = fp8_e4m3((x16 - sub[i % C]) * mul): the same with a per-channel centre (NHWC, C channels innermost; n % C == 0) */
int fr_quantize_f16_f8_centred(const void* x16, void* out8, int64_t n, int C, const float* sub, float mul,
                               fr_stream_t stream);
/* A run of `nblocks` stride-1 residual blocks at 14x14x256 (IResNet-100 stage 3 after its first block: 29 blocks =
 * 58 convs, 57 % of the network's FLOPs) as ONE launch with the image resident in LDS: one workgroup per image, a
 * conv's output overwrites its input in place, only the weights stream (conv_stage14.hip).  Same math as the
 * per-layer calls: block = conv3x3(+9-class border bias, PReLU) -> conv3x3(+bias) + input, f32 accumulation, one
 * rounding to f16 per conv output.  x: f16 NHWC [B,14,14,256] (input of the first block), y: same shape (the last
 * block's output; nothing else is written - the residual stream stays in LDS), x != y.  wstream: the convs' weights
 * in kernel order (conv1, conv2 of block 0, conv1 of block 1, ...), each re-ordered by fr_conv_stage14_pack from the
 * [256][9*256] f16 layout of fr_conv_nhwc_f16 into 72 x 16 KB slot images (fr_conv_stage14_weight_bytes(1) bytes per
 * conv).  params: f32
 * [2*nblocks][10][256]: rows 0..8 the bias of border class (row class * 3 + column class) - a conv with a plain bias
 * repeats it nine times - row 9 the PReLU slope (1.0 = none). */
size_t fr_conv_stage14_weight_bytes(int nconv);
int fr_conv_stage14_pack(const void* w, void* out, fr_stream_t stream);
int fr_conv_stage14_f16(const void* x, void* y, const void* wstream, const float* params, int B, int nblocks,
                        fr_stream_t stream);
/* The run of stride-1 128 -> 128 residual blocks of IResNet's 28x28 stage (r100: 12 blocks = 24 convs; embed half of
 * FaceAnalysis.get, /root/reference/infrenceServer.py:528) as ONE launch, one workgroup per face walking its own map through
 * all the convs (conv_stage28.hip): half an image per pass, the half's input halo in LDS, weights streaming, outputs
 * straight from the accumulators to HBM, read back by the same workgroup.  Same math as the blocks run through
 * fr_conv_nhwc_f16.  x: f16 [B][28][28][128], OVERWRITTEN with the run's output; mid: scratch of the same size; wstream: the
 * convs' weights in kernel order, each re-ordered by fr_conv_stage28_pack from the [128][9*128] f16 layout into 36 x 8 KB
 * slot images (fr_conv_stage28_weight_bytes(1) bytes per conv); params: f32 [2*nblocks][10][128] = 9 border-class biases
 * (a plain bias nine times) + PReLU slope (1.0 = none). */
size_t fr_conv_stage28_weight_bytes(int nconv);
int fr_conv_stage28_pack(const void* w, void* out, fr_stream_t stream);
int fr_conv_stage28_f16(void* x, void* mid, const void* wstream, const float* params, int B, int nblocks, fr_stream_t stream);
/* 3x3 / stride 1 / pad 1 conv with 64 input channels on square images whose side is a multiple of 28 (IResNet-100: 112x112 and
 * 56x56; embed half of FaceAnalysis.get, /root/reference/infrenceServer.py:528), one launch per layer: a workgroup walks one
 * face (x one 64-cout group) region by region (14 x 28 output pixels), the next region's input halo arriving in a second LDS
 * buffer under the current region's K loop (conv_walk64.hip).  Same arithmetic and argument meaning as fr_conv_nhwc_f16
 * (bias_mode 1 = nine border-class biases [9][Cout]); wstream: the [Cout][9*64] f16 weights re-ordered by
 * fr_conv_walk64_pack (fr_conv_walk64_weight_bytes(Cout) bytes); Cout % 64 == 0; y must not alias x; residual may alias y. */
size_t fr_conv_walk64_weight_bytes(int Cout);
int fr_conv_walk64_pack(const void* w, void* out, int Cout, fr_stream_t stream);
int fr_conv_walk64_f16(const void* x, const void* wstream, void* y, const float* bias, int bias_mode, const float* slope,
                       const void* residual, int B, int HW, int Cout, fr_stream_t stream);
/* The fp8 twin of fr_conv_stage14_f16 (BASELINE config C5): the same run of residual blocks on
 * v_mfma_scale_f32_16x16x128_f8f6f4, the conv inputs as centred e4m3 codes resident in LDS (conv_stage14_f8.hip).  Math and
 * operation order of fr_conv_nhwc_f8 per conv: acc * oscale + 9-class bias -> PReLU -> (+ f16 residual) -> one rounding to
 * f16 -> the next conv's codes fp8((y - mu_next) * inv_sx_next).  x8: e4m3 codes NHWC [B,14,14,256] of the first conv's
 * input, x16: the same tensor in f16 (the first block's residual), y16: f16, receives every block's output in turn (the
 * residual stream goes through HBM: it does not fit beside the codes and the weight ring), x16 != y16.  wstream: the
 * convs' e4m3 weights [256][9*256] re-ordered by fr_conv_stage14_f8_pack into 18 x 32 KB slot images each
 * (fr_conv_stage14_f8_weight_bytes(1) bytes per conv).  params: f32 [2*nblocks][14][256]: row 0 oscale, 1 its reciprocal,
 * 2..10 the nine border-class biases, 11 the PReLU slope (1.0 = none), 12 mu of the NEXT conv's input, 13 whose first
 * element is 1 / sx of the next conv (fr_conv_stage14_f8_param_floats() floats per conv). */
size_t fr_conv_stage14_f8_weight_bytes(int nconv);
size_t fr_conv_stage14_f8_param_floats(void);
int fr_conv_stage14_f8_pack(const void* w8, void* out, fr_stream_t stream);
int fr_conv_stage14_f8(const void* x8, const void* x16, void* y16, const void* wstream, const float* params, int B,
                       int nblocks, fr_stream_t stream);
/* Calibration-time weight rounding for fr_conv_nhwc_f8 (GPTQ, Frantar et al. 2022): W f64 [rows][K] folded weights,
 * U f64 [K][K] = upper Cholesky factor of the inverse of the second-moment matrix of the conv's input patches (K order
 * as W's columns), sw f32 [rows] the per-row scale.  Q f32 [rows][K] receives values ON THE e4m3 GRID (w8 = Q exactly):
 * column k is rounded to the nearest sw * e4m3 value (ties to even, saturating) and its error is pushed onto the
 * columns still to come along row k of U, so that the conv OUTPUT error is what is minimised.  K <= 8192. */
int fr_gptq_round_e4m3(const double* W, const double* U, const float* sw, float* Q, int rows, int K, fr_stream_t stream);
/* Split-K tail of an ordinary conv (small batches): y = epi(sum_z partial[z]) with the epilogue of fr_conv_nhwc_f16
 * (bias or 9-class border bias, PReLU, residual, one rounding to f16).  partial: f32 [splitk][M][Cout]. */
int fr_conv_splitk_epilogue(const float* partial, int splitk, int M, int Cout, int Ho, int Wo,
                            const float* bias, int bias_mode, const float* slope, const void* residual,
                            void* y, fr_stream_t stream);
/* 3x3 / stride 1 / pad 1 conv of a forward of one to eight faces (single frames; same reference site, infrenceServer.py:528),
 * split along K INSIDE a workgroup: sixteen waves share one 16- (past 256 workgroups 32-, then 64-) pixel x 32-cout output tile, a sixteenth of K each, partials
 * summed through LDS in wave order, then the fused epilogue of fr_conv_nhwc_f16 ((border-class) bias -> PReLU -> + residual
 * -> one rounding to f16) - ONE launch where the split-K mode of fr_conv_nhwc_f16 + fr_conv_splitk_epilogue are two
 * (conv_inblock.hip).  Takes fr_conv_args with KH = KW = 3, stride 1, pad 1, Cin % 32 == 0, Cin <= 512, Cout % 32 == 0,
 * x2 / out_f32_partial NULL; splitk is ignored.  Differs from the other modes by f32 summation order only. */
int fr_conv_inblock_f16(const fr_conv_args* args, fr_stream_t stream);
/* A prepared run of convs in ONE call (single frames are launch-bound from an interpreted host: ~100 convs of a few
 * microseconds each).  Step kind 0: fr_conv_nhwc_f16(args).  Kind 1: the small-batch split-K form of the conv that
 * `args` describes as a whole (x, w, y, bias, bias_mode, slope, residual, splitk > 1, out_f32_partial = scratch of
 * splitk * M * Cout floats): the partials launch followed by fr_conv_splitk_epilogue into args.y.  Kind 2:
 * fr_conv_inblock_f16(args).  Same kernels, same order, same bits as the individual calls; stops at the first failing step. */
typedef struct {
    int kind;
    fr_conv_args args;
} fr_conv_step;
int fr_conv_sequence(const fr_conv_step* steps, int nsteps, fr_stream_t stream);
/* FC tail: sum split-K partials + bias -> embedding f32 [B,dim]; then
 * normed_embedding = embedding / ||embedding|| (Face.normed_embedding, infrenceServer.py:532) */
int fr_fc_reduce_l2norm(const float* partial, int splitk, int B, int dim, const float* bias,
                        float* embedding, float* normed, fr_stream_t stream);


/* ---------------------------------------------------------------- align ----
 * a-3  5-point similarity (closed-form least squares == Umeyama for proper rotations) and
 * bilinear warpAffine to size x size, border 0, uint8 rounding, then (x-127.5)/127.5,
 * BGR->RGB, NHWC f16 with C padded to 8 (the stem conv's packed input).  Stands in for
 * insightface face_align.norm_crop inside FaceAnalysis.get (infrenceServer.py:528).
 * frames: u8 [nframes,H,W,3] BGR; kps f32 [F,5,2]; frame_idx i32 [F]; count: device i32 (faces
 * at index >= *count are zero-filled) or NULL; out_u8_bgr u8 [F,size,size,3] and
 * M_out f32 [F,2,3] are optional. */
int fr_warp_affine_5pt(const uint8_t* frames, int nframes, int H, int W, const float* kps,
                       const int32_t* frame_idx, const int32_t* count, int F, int size,
                       void* out_f16_nhwc8, uint8_t* out_u8_bgr, float* M_out, fr_stream_t stream);

/* fixed-shape form: kps f32 [nframes*cap,5,2] in per-frame slots, counts i32 [nframes] on the device; slot
 * (frame, j) is warped iff j < counts[frame], else zero-filled: no host sync between detect and embed. */
int fr_warp_affine_5pt_slots(const uint8_t* frames, int nframes, int H, int W, const float* kps,
                             const int32_t* counts, int cap, int size, void* out_f16_nhwc8,
                             fr_stream_t stream);

/* Ragged batches: frames of differing sizes, each described by one 32-byte entry of a DEVICE table.  data: u8 [H,W,3] BGR
 * (device memory, any byte alignment); nh x nw: the size the frame takes on a detection canvas (fr_letterbox_u8; the warps
 * below do not read them).  Nothing outside [data, data + H*W*3) is read. */
typedef struct {
    const uint8_t* data;
    int32_t H, W, nh, nw;
    int32_t reserved[2];
} fr_frame_ref;
/* The two warps above over a frame table in place of (frames, nframes, H, W): frame_idx / the slot's frame number index
 * `refs`.  Same kernel body, same arithmetic: a face gives the bits fr_warp_affine_5pt gives for its frame alone. */
int fr_warp_affine_5pt_refs(const fr_frame_ref* refs, int nframes, const float* kps, const int32_t* frame_idx,
                            const int32_t* count, int F, int size, void* out_f16_nhwc8, uint8_t* out_u8_bgr,
                            float* M_out, fr_stream_t stream);
int fr_warp_affine_5pt_slots_refs(const fr_frame_ref* refs, int nframes, const float* kps, const int32_t* counts,
                                  int cap, int size, void* out_f16_nhwc8, fr_stream_t stream);

/* --------------------------------------------------------------- detect ----
 * a-2  MTCNN cascade (detector half of FaceAnalysis.get, infrenceServer.py:528); the
 * conventions (resize, ordering, capacities) are those of oracle/detect.py. */
/* pyramid level: bilinear resize (half-pixel centres) + BGR->RGB + (x-127.5)*0.0078125 -> f32 NHWC(3) */
int fr_pyramid_resize_norm(const uint8_t* frames, int nframes, int H, int W, int hs, int ws,
                           float* out, fr_stream_t stream);
/* direct valid conv, f32 NHWC, + bias + PReLU (slope may be NULL).  w: [KH][KW][Cin][CoutP] with
 * CoutP = Cout rounded up to 16 (or 32), zero padded; bias/slope: [CoutP].
 * pool2 != 0: fused 2x2/s2 ceil-mode max pool after the PReLU (P-Net conv1).
 * nhead == 6: fused 1x1 head after the PReLU (P-Net conv3 -> conv4_1|conv4_2):
 * y = [.., 6] = head_b + act . head_w[32][6]. */
int fr_dconv_f32(const float* x, const float* w, const float* bias, const float* slope, float* y,
                 int B, int H, int W, int Cin, int Cout, int CoutP, int KH, int KW, int pool2,
                 const float* head_w, const float* head_b, int nhead, fr_stream_t stream);
/* MTCNN layers as LDS-tiled implicit GEMMs on v_mfma_f32_16x16x4_f32 (exact f32), the product path
 * of the detector.  `layer` selects a fixed geometry, with the following max pool FUSED where the net has one:
 * 0/1/2 = P-Net conv1(+PReLU+2x2 pool) / conv2 / conv3(+heads: y = [..,6]);
 * 10..14 = R-Net conv1(+3x3/s2 pool), conv2(+3x3/s2 pool), conv3, dense4, dense5_1|5_2;
 * 20..25 = O-Net conv1(+pool), conv2(+pool), conv3(+2x2 pool), conv4, dense5, dense6_1|6_2|6_3.
 * x f32 NHWC [B,H,W,Cin]; w packed [cout_group][tap][CinP][CP] (mtcnn.py _MConv); bias/slope padded to
 * the group size; slope NULL = no PReLU.  Channel counts are padded to multiples of 4 (P-Net conv1 writes
 * 12 channels, R/O-Net conv1 read 4).  Layer 0 takes `frames` (u8 BGR [B,FH,FW,3]) instead of x: the
 * pyramid level (H x W) is resized on the fly inside the tile load, with the same arithmetic as
 * fr_pyramid_resize_norm.  Blocks walk several tiles, prefetching the next tile into registers.
 * Layer 0 runs as its own kernel on v_mfma_f32_4x4x1 with a broadcast weight operand (pnet_conv1.hip: K = 27
 * exactly, one pixel per lane; needs slope != NULL); layer 3 is the same layer on the 16x16x4 form with the same
 * arguments and bit-identical outputs (same fma chain), kept for the A/B and the equality test.
 * counts / cap (R-/O-Net layers, optional): the batch is B / cap frames x cap crop slots and slot j of frame f
 * holds a candidate iff j < counts[f] (device i32); blocks that cover empty slots only do no work and leave those
 * outputs unwritten.  NULL: every image is computed.
 * y_split (layer 0 only, optional): a second copy of the output as split f16, 64 B per pixel = [hi ch0-7 | hi ch8-15 |
 * lo ch0-7 | lo ch8-15] with x = hi + lo and channels 12-15 zero - the operand format of fr_pnet23_split_f16. */
int fr_dconv_mfma_f32(int layer, const float* x, const float* w, const float* bias, const float* slope,
                      float* y, int B, int H, int W, const float* head_w, const float* head_b,
                      const uint8_t* frames, int FH, int FW, const int32_t* counts, int cap, void* y_split,
                      fr_stream_t stream);
/* R-Net / O-Net first layer fused with the crop that feeds it (net 0: 24x24 crop -> conv 3->28 -> PReLU -> 3x3/s2 ceil
 * pool -> y f32 [nframes*cap, 11, 11, 28]; net 1: 48x48 -> conv 3->32 -> ... -> [nframes*cap, 23, 23, 32]): the
 * arithmetic of fr_crop_resize_norm followed by layer 10 / 20 of fr_dconv_mfma_f32, bit for bit, without the crop
 * tensor in HBM.  boxes f32 [nframes*cap, 4] (trunc'ed inside), counts i32 [nframes]: slot j of frame f is computed
 * iff j < counts[f], other outputs stay unwritten.  w f32 [27][Cout]: k = (kh*3 + kw)*3 + channel (R, G, B);
 * bias / slope f32 [Cout]. */
int fr_crop_conv1_f32(int net, const uint8_t* frames, int nframes, int H, int W, const float* boxes,
                      const int32_t* counts, int cap, const float* w, const float* bias, const float* slope,
                      float* y, fr_stream_t stream);
/* The same layer with its pooled map written as SPLIT f16 (x = hi + lo, hi = f16(x), lo = f16(x - hi)):
 * y_split [nframes*cap][P*P pixels][hi 32 channels | lo 32 channels], 128 B per pixel, channels >= Cout zero (P = 11 / 23) -
 * the operand format of fr_ro_conv2_split.  Same slots computed / left unwritten as fr_crop_conv1_f32.
 * conv_f16 = 0: the conv itself is the f32 form's (the map is hi + lo of fr_crop_conv1_f32's to 2^-21); 1: the conv runs on
 * the f16 matrix cores with split-precision operands too (the split format's error from the f32 form: DESIGN.md 4.3a); the
 * O-Net's batch launch (several slots per block) then takes the STRIP form: a wave walks a strip of 16 conv columns down the
 * crop and pools the raw sums in registers, no conv map in LDS; 2: the same arithmetic in the TILE form everywhere (bands of
 * conv rows through an LDS tile, pooled from there) - the same bytes as 1, kept for the A/B and the bit-equality test.  The
 * R-Net and every launch of one slot per block run the tile form under 1 as well (the R-Net's strip form measured slower).
 * | FR_RC1_BATCH_SHAPE: take the several-slots-per-block launch whatever the slot count (by default only from 8192 / 2048
 * slots on) - how a small test reaches the batch kernels. */
#define FR_RC1_BATCH_SHAPE 16
int fr_crop_conv1_split(int net, const uint8_t* frames, int nframes, int H, int W, const float* boxes,
                        const int32_t* counts, int cap, const float* w, const float* bias, const float* slope,
                        void* y_split, int conv_f16, fr_stream_t stream);
/* fr_crop_conv1_f32 for a compact LIST of slots: row i of y is the f32 map of slot list[i], i < min(*list_count, list_cap)
 * (device-side count; boxes / frames are indexed by list[i], frame = list[i] / cap). */
int fr_crop_conv1_list_f32(int net, const uint8_t* frames, int nframes, int H, int W, const float* boxes, int cap,
                           const int32_t* list, const int32_t* list_count, int list_cap, const float* w,
                           const float* bias, const float* slope, float* y, fr_stream_t stream);
/* R-Net / O-Net SECOND layer on the f16 matrix cores with split-precision operands (three v_mfma_f32_16x16x32_f16 per
 * product term, f32 accumulate; heads differ from the f32 layers by the split format's error): net 0: [.,11,11,28] -> conv 3x3 -> PReLU ->
 * 3x3/s2 pool -> y f32 [nslots,4,4,48]; net 1: [.,23,23,32] -> ... -> [nslots,10,10,64] - the outputs of layers 11 / 21 of
 * fr_dconv_mfma_f32.  x_split: fr_crop_conv1_split's map; w f32 [Cout][9 taps][32 channels] (channels >= Cin zero);
 * counts / cap as fr_dconv_mfma_f32 (nslots = frames x cap).  The cascade's keep / reject decisions stay those of f32
 * arithmetic through the exact pass below.  zero_word (optional): a device int32 the kernel clears - the list counter of
 * the fr_ro_margin_list call that follows in the stream (saves a memset launch). */
int fr_ro_conv2_split(int net, const void* x_split, const float* w, const float* bias, const float* slope, float* y,
                      int nslots, const int32_t* counts, int cap, int32_t* zero_word, fr_stream_t stream);
/* The small tail layers of R-Net / O-Net as one split-precision GEMM kernel on the f16 matrix cores (x = hi + lo in f16,
 * three MFMAs per product term, f32 accumulate; the split format's error from the f32 layers): layer 12 = R-Net conv3
 * (2x2, 48 -> 64, [.,4,4,48] -> [.,3,3,64]), 13 = R-Net dense4 ([.,3,3,64] -> [.,128]), 22 = O-Net conv3 (3x3, 64 -> 64,
 * [.,10,10,64] -> 8x8 -> 2x2/s2 max pool -> [.,4,4,64]), 23 = O-Net conv4 (2x2, 64 -> 128,
 * [.,4,4,64] -> [.,3,3,128]), 24 = O-Net dense5 ([.,3,3,128] -> [.,256]) - the layers of the same ids of fr_dconv_mfma_f32,
 * + bias + PReLU.  w_packed: fr_ro_gemm_pack(layer, w) of the f32 weights [Cout][K], K = (kh, kw, channel) ascending
 * (fr_ro_gemm_weight_bytes(layer) bytes).  counts / cap as fr_dconv_mfma_f32.  Batch path only: see fr_ro_conv2_split. */
size_t fr_ro_gemm_weight_bytes(int layer);
int fr_ro_gemm_pack(int layer, const float* w, void* out, fr_stream_t stream);
int fr_ro_gemm_split(int layer, const float* x, const void* w_packed, const float* bias, const float* slope, float* y,
                     int nslots, const int32_t* counts, int cap, fr_stream_t stream);
/* The exact pass's work list: the valid slots whose logit difference head[s][1] - head[s][0] lies within `margin` of
 * logit_thr = ln(t / (1 - t)) (t: the stage's probability threshold), or whose heads are not all finite (NaN or +-inf: an
 * f16 operand overflowed), are appended to list (any order); *list_count = how
 * many there are (may exceed list_cap: entries past it are dropped, consumers clamp).  head f32 [nframes*cap][nhead].
 * *list_count must be 0 on entry (fr_ro_conv2_split's zero_word, or the caller's memset).
 * OVERFLOW (*list_count > list_cap): list holds list_cap distinct qualifying slots, which ones is unspecified (atomic order);
 * *list_count is still the full number of qualifying slots.  The slots dropped past list_cap keep their split-precision heads -
 * their threshold decision is then NOT the f32 one.  Nothing signals it on the device; a caller that must know compares
 * *list_count with list_cap after the cascade (MTCNNHIP.exact_list_overflow(): per thread, every frame group of a call; the
 * batch-path tests and bench.py's line do) and raises list_cap or re-runs the stage on the f32 layers.
 * The f32 layers that follow take the list's own counter as their `counts` with cap = list_cap: fr_dconv_mfma_f32 and
 * fr_ro_gemm_split only test slot < counts[f], so a counter ABOVE list_cap is tolerated there (every one of the list_cap rows
 * is computed, none beyond). */
int fr_ro_margin_list(const float* head, int nhead, const int32_t* counts, int nframes, int cap, float logit_thr,
                      float margin, int32_t* list, int32_t* list_count, int list_cap, fr_stream_t stream);
/* dst[list[i]][:] = src[i][:] for i < min(*list_count, list_cap): the exactly re-evaluated head rows go back to their slots. */
int fr_ro_scatter_rows(const float* src, const int32_t* list, const int32_t* list_count, int list_cap, int ncols,
                       float* dst, fr_stream_t stream);
/* P-Net conv2 -> PReLU -> conv3 -> PReLU -> heads fused, on the f16 matrix cores with split-precision operands
 * (x = hi + lo in f16, three MFMAs per product term, f32 accumulate; the split format's logit error), followed by an EXACT f32
 * re-evaluation of every cell whose logit1 - logit0 >= refine_logit_thr (pass ln(t/(1-t)) - 2e-3 for threshold t):
 * every cell that can be kept by fr_pnet_candidates then carries exact f32 logits and regressions, every other cell is
 * below the threshold by more than the approximation error.  x1: P-Net conv1 output (layer 0 of fr_dconv_mfma_f32),
 * f32 [B,H1,W1,12]; w2 [16][10][16] / w3 [32][10][16]: (cout, tap, channel) with tap 9 and unused channels zero;
 * x1s: the same map as split f16 (y_split of layer 0), streamed into LDS by LDS-DMA.
 * b/s: bias and PReLU slope; hw [32][6], hb [6]: conv4_1|conv4_2.  head: f32 [B,H1-4,W1-4,6].
 * all_heads: 0 = only the rows of re-evaluated cells are written (all fr_pnet_candidates reads when it is given the
 * workspace as `dl` and refine_logit_thr as `dl_min`); 1 = the approximate heads of every other cell too (tests, traces).
 * refine_band_hi: <= refine_logit_thr (pass -INFINITY): as above.  > refine_logit_thr: only the cells with refine_logit_thr <=
 * logit1 - logit0 <= refine_band_hi - the band around the face threshold, pass ln(t/(1-t)) + 2e-3 - are re-evaluated
 * exactly (every keep / reject decision is still that of f32 arithmetic); the cells above the band keep their
 * split-precision rows, which the kernel then writes for every cell >= refine_logit_thr (the split format's error from the f32 heads).
 * refined_count (optional device i32, accumulated): number of re-evaluated cells.
 * workspace: fr_pnet23_workspace_bytes(B, H1, W1) bytes; its first B*(H1-4)*(W1-4) floats are the logit differences
 * (the `dl` argument of fr_pnet_candidates), behind them the per-block lists of the cells the exact pass re-evaluates.
 * all_heads bit 1 (value 2): the exact pass is NOT launched here - fr_pnet_finish_levels runs it for every level at once. */
size_t fr_pnet23_workspace_bytes(int B, int H1, int W1);
int fr_pnet23_split_f16(const float* x1, const void* x1s, int B, int H1, int W1, const float* w2, const float* b2, const float* s2,
                        const float* w3, const float* b3, const float* s3, const float* hw, const float* hb,
                        float* head, int all_heads, float refine_logit_thr, float refine_band_hi, int32_t* refined_count,
                        void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* The same post-state as fr_pnet23_split_f16 - dl, head rows, per-block lists and counts, the exact pass unless all_heads & 2 -
 * in two tiers: a COARSE pass over every cell with the hi halves of the operands only (one MFMA per product, no lo plane moved),
 * which writes its logit difference and lists every cell with dl >= refine_logit_thr - coarse_margin or a non-finite dl, and the
 * split-precision re-evaluation of the listed cells with the operand composition of fr_pnet23_split_f16, whose bits they then
 * carry.  Every cell fr_pnet23_split_f16 would list, or write a head row for, is re-evaluated while coarse_margin >= the hi-only
 * format's error of dl; the other cells hold a dl < refine_logit_thr, which is all that is ever asked of them.
 * coarse_margin = INFINITY re-evaluates every cell.  all_heads & 1 is refused (FR_E_INVALID): the approximate heads of every
 * cell are the split kernel's business.  coarse: fr_pnet23_coarse_workspace_bytes(B, H1, W1) bytes = [512 counts | the blocks'
 * coarse list segments].  visited_count (optional device i32, accumulated): cells on the coarse lists. */
size_t fr_pnet23_coarse_workspace_bytes(int B, int H1, int W1);
int fr_pnet23_coarse_f16(const float* x1, const void* x1s, int B, int H1, int W1, const float* w2, const float* b2, const float* s2,
                         const float* w3, const float* b3, const float* s3, const float* hw, const float* hb,
                         float* head, int all_heads, float refine_logit_thr, float refine_band_hi, int32_t* refined_count,
                         void* workspace, size_t workspace_bytes, float coarse_margin, void* coarse, size_t coarse_bytes,
                         int32_t* visited_count, fr_stream_t stream);
/* max pool, ceil mode, f32 NHWC */
int fr_maxpool_f32(const float* x, float* y, int B, int H, int W, int C, int k, int stride,
                   fr_stream_t stream);
/* P-Net level -> per-frame candidate lists: head f32 [nframes,hc,wc,6] = (logit0, logit1, reg0..3);
 * keeps cells with softmax face prob >= thr in raster order (first `cap`), emitting
 * box = floor((2*cell + {1,12}) / scale), score, reg.  boxes [nframes,cap,4], scores [nframes,cap],
 * regs [nframes,cap,4], counts i32 [nframes]; block_counts: i32 scratch [nframes*ceil(hc*wc/256)];
 * prob_out (optional) f32 [nframes,hc,wc].  dl / dl_min (optional, with fr_pnet23_split_f16): f32 [nframes,hc,wc]
 * approximate logit1 - logit0; cells with dl < dl_min are known to be below the threshold and their head rows are
 * not read (pass the workspace of fr_pnet23_split_f16 and its refine_logit_thr). */
int fr_pnet_candidates(const float* head, int nframes, int hc, int wc, float scale, float thr, int cap,
                       float* boxes, float* scores, float* regs, int32_t* counts,
                       int32_t* block_counts, float* prob_out, const float* dl, float dl_min, fr_stream_t stream);
/* per-list sort (descending score, ties by slot) + greedy NMS (mode 0: IoU, 1: IoMin).
 * Input list l = nseg segments of seg_cap slots (segment s at list index l*nseg+s, or s*L+l when
 * seg_major), counts i32 [L*nseg] (nseg*seg_cap <= 4096);
 * aux f32 [.., naux] rides along.  Output: first max_keep survivors in score order,
 * boxes_out [L,cap_out,4], scores_out [L,cap_out], aux_out [L,cap_out,naux], counts_out [L]. */
int fr_sort_nms(const float* boxes, const float* scores, const float* aux, int naux,
                const int32_t* counts, int L, int nseg, int seg_cap, int seg_major, float thr, int mode,
                int max_keep,
                float* boxes_out, float* scores_out, float* aux_out, int32_t* counts_out,
                int cap_out, fr_stream_t stream);
/* box refinement in place, regs = aux[..,0:4]: mode 0 = stage-1 regression (w = x2-x1) + square;
 * mode 1 = bbreg (w = x2-x1+1) + square; mode 2 = bbreg only. */
int fr_box_refine(float* boxes, const float* aux, int naux, const int32_t* counts, int L, int cap,
                  int mode, fr_stream_t stream);
/* zero-padded crop of trunc(box) (1-based inclusive) + bilinear resize to size x size + normalise
 * -> f32 NHWC [nframes*cap,size,size,4] (RGB + a zero channel); slots >= count are zero-filled. */
int fr_crop_resize_norm(const uint8_t* frames, int nframes, int H, int W, const float* boxes,
                        const int32_t* counts, int cap, int size, float* out, fr_stream_t stream);
/* R/O-Net decision: head f32 [L*cap,nh] = (logit0, logit1, reg0..3[, lm0..9]); keeps slots with
 * softmax face prob > thr in slot order, emitting trunc(box), score, aux = (reg0..3[, landmarks
 * (x1,y1)..(x5,y5) in frame coordinates]) (nh,naux) = (6,4) or (16,14). */
int fr_stage_select(const float* boxes, const float* head, int nh, const int32_t* counts, int L, int cap,
                    float thr, float* boxes_out, float* scores_out, float* aux_out, int naux,
                    int32_t* counts_out, float* prob_out, fr_stream_t stream);

/* Band mode with conv1 on the f16 matrix cores (round 4, batches).  fr_pnet_conv1_band mode 0: P-Net conv1 (+ the pyramid
 * resize, PReLU, 2x2 ceil pool: layer 0 of fr_dconv_mfma_f32) with split-precision operands - writes the split map y_split
 * only (y optional: the f32 view of the same split-accurate values).  The exact pass then needs an exact f32 map under the
 * windows of the cells on its lists: fr_pnet_band_tiles marks the conv1 tiles (8 x 32 map pixels) those windows touch
 * (tbuf: 1 + ceil(tiles / 32) int32 = [count | bitmap], zeroed here; tiles: int32 [fr_pnet_band_tiles_count(B, H1, W1)]), and
 * fr_pnet_conv1_band mode 1 runs the EXACT f32 kernel over that list (list = tiles, list_count = tbuf, list_cap = the tile
 * count), writing y for those tiles only.  Call order per level: mode 0, fr_pnet23_split_f16 (all_heads | 2, band), band_tiles,
 * mode 1, fr_pnet_finish_levels (one level).  H, W: the level's size; H1, W1: the conv1 map's. */
int fr_pnet_conv1_band(int mode, const uint8_t* frames, int B, int FH, int FW, int H, int W, const float* w, const float* bias,
                       const float* slope, float* y, void* y_split, const int32_t* list, const int32_t* list_count, int list_cap,
                       fr_stream_t stream);
size_t fr_pnet_band_tiles_count(int B, int H1, int W1);
int fr_pnet_band_tiles(const void* workspace, int B, int H1, int W1, int32_t* tbuf, int32_t* tiles, fr_stream_t stream);
/* The exact pass (deferred by all_heads bit 1) and fr_pnet_candidates for ALL pyramid levels of a batch in three launches
 * instead of three per level: the same cells, the same ordered compaction per level and frame.  A level entry repeats what
 * its fr_pnet23_split_f16 / fr_pnet_candidates calls would have been given (workspace = that level's, unchanged since;
 * block_counts: i32 [nframes * ceil((H1-4)*(W1-4)/256)]).  At most 16 levels. */
typedef struct {
    const float* x1; float* head; void* workspace;
    int H1, W1; float scale;
    float* boxes; float* scores; float* regs; int32_t* counts; int32_t* block_counts;
    /* the pyramid descriptor of the fr_pnet_pyramid_* launches (fr_pnet_finish_levels does not read these) */
    void* x1s;            /* the split conv1 map [nframes, H1, W1, 64 B] */
    int hs, ws;           /* the level's size (the frame is resized to it inside conv1's tile load) */
    int f16;              /* != 0: conv1 in its f16 form (split map only) + exact f32 tiles under the band cells' windows */
} fr_pnet_level;
int fr_pnet_finish_levels(const fr_pnet_level* levels, int nlevels, int nframes, const float* w2, const float* b2,
                          const float* s2, const float* w3, const float* b3, const float* s3, const float* hw,
                          const float* hb, float thr, int cap, float dl_min, int32_t* refined_count, fr_stream_t stream);
/* The P-Net of a whole pyramid with each layer launched ONCE (batches): a block of a launch finds its level in a table built
 * from `levels` (largest level first) and runs what the level's own launch would have run - every value is bit for bit that of
 * the per-level calls above.  Every entry carries x1, x1s, hs, ws, H1 = (hs - 1) / 2, W1 = (ws - 1) / 2, head and the level's own
 * workspace (fr_pnet23_workspace_bytes).  Call order: fr_pnet_pyramid_conv1 mode 0 (the f16 form over the levels with f16 != 0 -
 * split map only - and the f32 form over the others: x1 and x1s), fr_pnet_pyramid_p23 (fr_pnet23_split_f16 of every level, the
 * exact pass deferred), then - when some level has f16 != 0 - fr_pnet_pyramid_band_tiles (tbuf: int32 [1 + sum over those levels
 * of ceil(fr_pnet_band_tiles_count / 32)] = [count | bitmaps], zeroed here; tiles: int32 [sum of fr_pnet_band_tiles_count],
 * entries level << 27 | tile) and fr_pnet_pyramid_conv1 mode 1 (list = tiles, list_count = tbuf, list_cap = the capacity of
 * `tiles`: the exact f32 form over those tiles, x1 of the f16 levels is written inside them only), and fr_pnet_finish_levels. */
int fr_pnet_pyramid_conv1(int mode, const uint8_t* frames, int B, int FH, int FW, const fr_pnet_level* levels, int nlevels,
                          const float* w, const float* bias, const float* slope, const int32_t* list, const int32_t* list_count,
                          int list_cap, fr_stream_t stream);
int fr_pnet_pyramid_p23(const fr_pnet_level* levels, int nlevels, int nframes, const float* w2, const float* b2, const float* s2,
                        const float* w3, const float* b3, const float* s3, const float* hw, const float* hb, int all_heads,
                        float refine_logit_thr, float refine_band_hi, fr_stream_t stream);
int fr_pnet_pyramid_band_tiles(const fr_pnet_level* levels, int nlevels, int nframes, int32_t* tbuf, int32_t* tiles, fr_stream_t stream);
/* fr_pnet_pyramid_p23 in the two tiers of fr_pnet23_coarse_f16, one launch each over all levels: the same post-state.
 * coarse[l]: level l's coarse buffer (fr_pnet23_coarse_workspace_bytes(nframes, H1, W1) bytes), beside the level table. */
int fr_pnet_pyramid_p23_coarse(const fr_pnet_level* levels, int nlevels, int nframes, const float* w2, const float* b2, const float* s2,
                               const float* w3, const float* b3, const float* s3, const float* hw, const float* hb, int all_heads,
                               float refine_logit_thr, float refine_band_hi, float coarse_margin, void* const* coarse,
                               int32_t* visited_count, fr_stream_t stream);

/* det_size: the detection canvas of insightface's FaceAnalysis.prepare(det_size=(dw, dh)) (the reference's prepare(ctx_id=0)
 * means 640 x 640, infrenceServer.py:416).  ONE launch for a ragged batch: frame f of `refs` is resized to refs[f].nh x
 * refs[f].nw - the pyramid's bilinear resize (f32, half-pixel centres, edge clamp: oracle/detect.py resize_bilinear) of the
 * BGR bytes, rounded floor(v + 0.5) and clamped to [0, 255] - and placed top-left on canvas[f] (u8 [nframes,dh,dw,3]); every
 * other byte of the canvas is written 0 by the same launch.  nh == H and nw == W is an exact copy.  1 <= nh <= dh,
 * 1 <= nw <= dw per entry (the host computes them: letterbox_geometry); entries outside that are clamped to the canvas.
 * dw % 16 == 0 takes 16-byte canvas stores, any other width byte stores. */
int fr_letterbox_u8(const fr_frame_ref* refs, int nframes, uint8_t* canvas, int dh, int dw, fr_stream_t stream);
/* Detections of the canvas back to frame pixels, in place: every coordinate of boxes f32 [nframes,cap,4] and kps f32
 * [nframes,cap,5,2] of the slots j < counts[f] is divided (IEEE f32) by det_scale[f]; other slots are left untouched. */
int fr_detections_unscale(float* boxes, float* kps, const int32_t* counts, const float* det_scale, int nframes, int cap,
                          fr_stream_t stream);

/* YUV 4:2:0 frames -> the packed BGR u8 [H,W,3] frames every entry above takes: what a video decoder produces (the reference's
 * live path is RTSP / webcam capture, infrenceServer.py:573-601; cv2.VideoCapture decodes to YUV 4:2:0 and converts on the CPU)
 * converted on the device, so a frame crosses the link at 1.5 bytes per pixel.  A source frame is u8 [H*3/2, W] (cv2's
 * convention), H and W even:
 *   FR_YUV_NV12   Y plane [H,W], then H/2 rows of W bytes holding interleaved U, V
 *   FR_YUV_I420   Y plane [H,W], then the U plane [H/2,W/2], then the V plane [H/2,W/2]
 * Nearest chroma (the 2x2 pixel block (2i..2i+1, 2j..2j+1) shares chroma sample (i, j)) and, per pixel, in 32-bit integers:
 *   y = max(0, Y - y_off) * cy + (1 << 19);   u = U - 128;   v = V - 128
 *   B = sat8((y + cub u) >> 20)   G = sat8((y + cug u + cvg v) >> 20)   R = sat8((y + cvr v) >> 20)
 * with an arithmetic shift (floor) and sat8 = clamp to [0, 255]: exact, the same bytes from any launch shape.  The constants
 * come from the caller, one set per colour matrix (the Python host's table: colour.MATRICES); they are refused unless
 * 0 <= y_off <= 255, cy >= 0 and 255 cy + 2^19 + 128 max(|cub|, |cug| + |cvg|, |cvr|) < 2^31 - no intermediate leaves int32.
 * Any byte alignment of the frames; W % 16 == 0 with frames that start on 16 bytes gives aligned 16-byte accesses throughout.
 * One launch each; nothing outside the source and destination frames is read or written.
 *
 * fr_yuv420_to_bgr_u8: a uniform batch, source frames back to back at H*W*3/2 bytes each, destination frames at H*W*3 each.
 * Refused before any launch: odd or non-positive H or W, a frame of 2 GiB or more (H*W*3 >= 2^31), an unknown layout, bad
 * constants, a null pointer with N > 0.  N == 0 returns FR_OK and reads nothing.
 * fr_yuv420_to_bgr_refs_u8: frames of differing sizes.  dst_refs: a DEVICE table whose entry f names destination frame f
 * (data - written here, the const of the struct notwithstanding -, H, W; nh / nw are not read: the table a RaggedIngest hands
 * to the warps and the letterbox serves as it is); src_ptrs: a DEVICE array of nframes pointers, src_ptrs[f] the YUV frame of
 * entry f (dst_refs[f].H * W * 3 / 2 bytes).  The sizes live on the device, so they cannot be refused here: an entry with an
 * odd or non-positive side, of 2 GiB or more, or with a null pointer on either side is skipped as a whole (the host checks:
 * colour.check_yuv_shape).  nframes == 0 returns FR_OK and reads nothing; at most 65535 frames. */
#define FR_YUV_NV12 0
#define FR_YUV_I420 1
int fr_yuv420_to_bgr_u8(const uint8_t* src, uint8_t* dst, int N, int H, int W, int layout, int y_off, int cy, int cub, int cug,
                        int cvg, int cvr, fr_stream_t stream);
int fr_yuv420_to_bgr_refs_u8(const fr_frame_ref* dst_refs, const uint8_t* const* src_ptrs, int nframes, int layout, int y_off,
                             int cy, int cub, int cug, int cvg, int cvr, fr_stream_t stream);

/* Activity gate: which frames of a camera batch differ from the last PROCESSED frame of the same camera, so that the engine
 * pass can leave the others out (the reference takes every 2nd frame whatever it shows, peopleCount.py:938,962, and drops
 * frames when a queue is full, infrenceServer.py:595-598,614-617).  A frame is BGR u8 [H,W,3].  In 32-bit integers:
 *   L = (29 B + 150 G + 77 R + 128) >> 8                 per pixel, 0 .. 255 (the weights sum to 256)
 *   m = (sum of L over the cell + 128) >> 8              per 16 x 16 cell; gh = H / 16 rows of gw = W / 16 cells, row-major
 *                                                        (remainder rows and columns belong to no cell)
 * State lives on the device, per camera slot s < S, and belongs to the caller (zeroed once):
 *   grid u8 [S][C]     the cell means of the last frame of the slot that was judged active
 *   geom i32 [S][2]    the (H, W) grid[s] was taken at, (0, 0): none
 *   idle i32 [S]       consecutive frames judged inactive
 * Per frame f, with s = slot[f] and cur[f] = its cell means (u8 [N][C] scratch, written for every judged frame):
 *   changed[f] = -1 if geom[s] != (H, W), else the number of cells with |cur - grid[s]| > thr          (strictly greater)
 *   active[f]  = changed < 0 or changed >= min_cells or (max_idle > 0 and idle[s] >= max_idle)
 *   active: grid[s] = cur[f], geom[s] = (H, W), idle[s] = 0;   else idle[s] += 1 (grid and geom untouched).
 * A frame with H < 16 or W < 16, with more than C cells, or whose slot is outside [0, S) is active with changed = -1 and no
 * state is read or written for it.  slot, changed, active: i32 [N] on the device.  Two frames of one batch must not name one
 * slot (the result is then unspecified, every access still inside the arrays).
 * Two launches on `stream` (cell means: every byte of the cell area read once, any byte alignment; then one workgroup per
 * frame that counts, judges and commits), no synchronisation, allocation, memset or atomics: the same bytes from any launch
 * shape.
 *
 * fr_frame_activity_u8: a uniform batch u8 [N,H,W,3].  Refused before any launch: more than 65535 frames, non-positive H, W, S
 * or C, thr outside 0 .. 255, min_cells < 1, max_idle < 0, H*W*3 >= 2^31, a null pointer with N > 0.  N == 0 returns FR_OK
 * and touches nothing.
 * fr_frame_activity_refs_u8: the same over a DEVICE frame table (data, H and W are read; the table a RaggedIngest hands to the
 * letterbox serves as it is).  The sizes live on the device: an entry of 2 GiB or more or with a null pointer is treated as
 * one without cells (active, changed = -1, no state).  Added under ABI 106. */
int fr_frame_activity_u8(const uint8_t* frames, int N, int H, int W, const int32_t* slot, int S, uint8_t* grid, int32_t* geom,
                         int32_t* idle, int C, uint8_t* cur, int32_t* changed, int32_t* active, int thr, int min_cells,
                         int max_idle, fr_stream_t stream);
int fr_frame_activity_refs_u8(const fr_frame_ref* refs, int nframes, const int32_t* slot, int S, uint8_t* grid, int32_t* geom,
                              int32_t* idle, int C, uint8_t* cur, int32_t* changed, int32_t* active, int thr, int min_cells,
                              int max_idle, fr_stream_t stream);

/* Device HUD: the last stage of the live path (the reference's recognize_faces returns the frame with a HUD drawn on every face,
 * infrenceServer.py:418-513), drawn IN PLACE into BGR u8 frames on the device.  The picture is defined by
 * tests/helpers/hud_ref.py and reproduced byte for byte (32-bit integer arithmetic only): per pixel a fold over the frame's faces
 * in slot order and, within a face, over its layers.  Rectangles are inclusive on both ends; pixels outside the frame do not
 * exist.  With s = scale (every length constant is multiplied by it) and c the face's colour:
 *   1. box     [x1,x2] x [y1,y2] minus [x1+2s,x2-2s] x [y1+2s,y2-2s]:  p = (102 c + 154 p + 128) >> 8
 *   2. ticks   p = c; L = 15 s, h = s; per corner (cx, cy) of (x1,y1) (x2,y1) (x1,y2) (x2,y2), u = x - cx, v = y - cy:
 *              [cx,cx+L] x [cy-h,cy+h],  [cx-h,cx+h] x [cy,cy+L],  0 <= u,v <= L and |u + v - L| <= h
 *   3. bars    bx = x2 + 10 s.  Detection: outline [bx,bx+6s] x [y1,y2], s thick inward, (100,100,100); fill [bx,bx+6s] x
 *              [y2-dh,y2] in (255,140,0); glyph 'D', white, glyph scale s, top-left (bx-2s, y1-12s).  Recognition: the same at
 *              bx + 12 s, filled in c over rh rows, glyph 'R'.  A height of 0 still fills one row.
 *   4. panel   g = 2 s; pw = maxlen 6 g + 20 s, ph = nlines 18 s + 10 s; px = max(0, min(x1, W - pw)); py = max(0, y2 + 10 s),
 *              and py = max(0, y1 - ph - 10 s) if py + ph > H.  Background [px,px+pw] x [py,py+ph]:
 *              p = (205 * 30 + 51 p + 128) >> 8; border s thick inward in c; line i in white, glyph scale g, top-left
 *              (px + 10 s, py + s + 18 s i).
 * Text: font is a DEVICE table u8 [95][7], glyph (ch - 0x20) as seven row masks, bit 4 the leftmost of 5 columns (the host's
 * one table: hud_font.py; the library holds no copy).  A glyph pixel covers g x g pixels, a character cell is 6 g wide; a byte
 * outside 0x20 .. 0x7E is drawn as '?'.
 *
 * counts i32 [n]; faces i32 [n][cap][FR_HUD_K], one record per face:
 *   [0..3] x1 y1 x2 y2 (ordered by the host)   [4..6] B G R   [7] dh   [8] rh   [9] nlines (0 .. 4)
 *   [10..13] the lengths of the lines in bytes   [14..15] reserved, 0
 * text u8 [n][cap][4][max_chars].  Slots j >= counts[f] are never read (counts is clamped to 0 .. cap).  What a record holds is
 * normalised before it is drawn: coordinates clamped to +-2^20, colours modulo 256, dh / rh clamped to [0, max(y2 - y1, 0)],
 * nlines to 0 .. 4, lengths to 0 .. max_chars.
 * One launch, a gather over output pixels in tiles of 16 x 64; a tile that no face's extent (the bounding rectangle of its
 * layers) meets is neither read nor written, and a pixel no layer hits is not written.  Any byte alignment of the frames.
 *
 * fr_hud_draw_u8: a uniform batch u8 [N,H,W,3].  fr_hud_draw_refs_u8: a DEVICE frame table (data - written here, the const of
 * the struct notwithstanding -, H and W are read; the table a RaggedIngest hands out serves as it is); an entry with a
 * non-positive side, of 2 GiB or more or with a null pointer is skipped as a whole.  Refused before any launch: more than 65535
 * frames or a negative count of them, cap outside 1 .. FR_HUD_MAX_CAP, max_chars outside 1 .. FR_HUD_MAX_CHARS, scale outside
 * 1 .. 8, non-positive H or W, a frame of 2 GiB or more (H*W*3 >= 2^31), a null pointer with n > 0.  n == 0 returns FR_OK and
 * reads nothing.  Added under ABI 106: no existing signature changed. */
#define FR_HUD_K 16
#define FR_HUD_MAX_CAP 64
#define FR_HUD_MAX_CHARS 64
int fr_hud_draw_u8(uint8_t* frames, int N, int H, int W, const int32_t* counts, int cap, const int32_t* faces,
                   const uint8_t* text, int max_chars, const uint8_t* font, int scale, fr_stream_t stream);
int fr_hud_draw_refs_u8(const fr_frame_ref* refs, int nframes, const int32_t* counts, int cap, const int32_t* faces,
                        const uint8_t* text, int max_chars, const uint8_t* font, int scale, fr_stream_t stream);

/* Face redaction: rectangles of BGR u8 frames on the device pixelated or filled IN PLACE, behind the engine pass and in front of
 * fr_hud_draw_u8 and the JPEG encoder, so that no unmasked picture of a masked face leaves the device.  The picture is defined by
 * tests/helpers/redact_ref.py and reproduced byte for byte (32-bit integer arithmetic only):
 *   cells   block x block, anchored at the picture's origin: pixel (x, y) lies in cell (x / block, y / block); the cells of the
 *           last column and row are cut at W and H, so a cell has n = cw ch <= block^2 pixels
 *   held    a pixel is held when at least one of its frame's regions contains it; a region is an inclusive rectangle
 *           x1 y1 x2 y2, ordered by the host, anywhere (negative, past the picture; clamped to +-2^20)
 *   mode 0  pixelate: a held pixel takes, per channel, (S + n / 2) / n, S the sum of the ORIGINAL bytes of its whole cell - the
 *           cell's pixels that no region holds included
 *   mode 1  fill: a held pixel takes the colour bgr (B in bits 0 .. 7, G in 8 .. 15, R in 16 .. 23)
 * A pixel no region holds is never written.  The grid does not depend on the regions: overlapping regions, a region listed twice
 * and any order of the list give the bytes of the union.
 *
 * counts i32 [n]; regions i32 [n][cap][4].  Slots j >= counts[f] are never read (counts is clamped to 0 .. cap).
 * One launch on the caller's stream, nothing allocated, nothing synchronised, no global atomics.  Work is cut by cell: a tile is
 * block rows x block * (64 / block) pixels, owned by one workgroup that reads all of it before it stores any of it and reads
 * nothing else; a tile that no region meets is neither read nor written.  Any byte alignment of the frames.
 *
 * fr_redact_u8: a uniform batch u8 [N,H,W,3].  fr_redact_refs_u8: a DEVICE frame table (data - written here, the const of the
 * struct notwithstanding -, H and W are read); an entry with a non-positive side, of 2 GiB or more or with a null pointer is
 * skipped as a whole.  Refused before any launch: more than 65535 frames or a negative count of them, cap outside
 * 1 .. FR_REDACT_MAX_CAP, block outside 2 .. 64, mode other than 0 / 1, non-positive H or W, a frame of 2 GiB or more, a null
 * pointer with n > 0.  n == 0 returns FR_OK and reads nothing.  Added under ABI 106: no existing signature changed. */
#define FR_REDACT_MAX_CAP 64
int fr_redact_u8(uint8_t* frames, int N, int H, int W, const int32_t* counts, int cap, const int32_t* regions,
                 int block, int mode, uint32_t bgr, fr_stream_t stream);
int fr_redact_refs_u8(const fr_frame_ref* refs, int nframes, const int32_t* counts, int cap, const int32_t* regions,
                      int block, int mode, uint32_t bgr, fr_stream_t stream);

/* Face chips: a square around each face, cut out of the full-size BGR u8 frames on the device and resampled to size x size
 * bytes - the thumbnail of an unknown-person event, a recognition log or a watch-list dashboard - in front of the redactor and
 * the HUD draw, so that a chip shows the unmasked, undrawn pixels.  The picture is defined by tests/helpers/chip_ref.py and
 * reproduced byte for byte (integers only).
 *
 * chips i32 [F][4], one record per chip: frame, x0, y0, side - the square [x0, x0 + side) x [y0, y0 + side) of that frame, in
 * frame pixels, partly or wholly outside the frame if it likes; a pixel outside the frame reads as the colour bgr_fill (B in
 * bits 0 .. 7, G in 8 .. 15, R in 16 .. 23).  With L = side and S = size, on one axis output j weighs source position p
 * (relative to the square's origin):
 *   box      L >= S, the exact area average: a source pixel is S units long, an output pixel L;
 *            w = min((j + 1) L, (p + 1) S) - max(j L, p S) where that is positive; the weights of an output sum to T = L
 *   bilinear L < S, half-pixel centres: n = (2 j + 1) L - S, p = floor(n / 2 S) (toward minus infinity: -1 at the leading
 *            edge), t = n - 2 S p; taps p (weight 2 S - t) and p + 1 (weight t), NOT clamped to the square: -1 and L read the
 *            frame's own neighbouring pixels, or the fill colour outside the frame; T = 2 S
 *   byte     (sum_y sum_x w_y w_x pix + T^2 / 2) / T^2 per channel, T^2 / 2 an integer division: round half up, the identity
 *            at L == S.  The largest sum, 255 * 4096^2 + 4096^2 / 2, fits an UNSIGNED 32-bit accumulator and no signed one.
 * Limits: 1 <= side <= FR_CHIP_MAX_SIDE, 16 <= size <= 256, |x0|, |y0| <= 2^20.  Records are device data and are checked on the
 * device: a record whose frame index is outside the batch, whose side is out of range, with a coordinate beyond the limit, or
 * whose frame-table entry is null, non-positive or of 2 GiB or more gives a chip of pure fill colour - never a fault, never a
 * gap in out.
 *
 * One launch on the caller's stream (grid: chip x band of output rows), nothing allocated, nothing synchronised, no global state.
 * Nothing outside [data, data + H*W*3) of a frame is read - any byte alignment of the frames and their rows - and nothing outside
 * out[0 : F * size * size * 3) is written.
 *
 * fr_face_chips_u8: a uniform batch u8 [N,H,W,3].  fr_face_chips_refs_u8: a DEVICE frame table (data, H and W are read; the
 * table a RaggedIngest hands out serves as it is).  Refused before any launch: N / nframes outside 0 .. 65535, non-positive H or
 * W, a frame of 2 GiB or more, F outside 0 .. 2^20, size outside 16 .. 256, a null pointer with F > 0 (frames / refs may be null
 * with no frames: every chip is fill then).  F == 0 returns FR_OK and reads nothing.  Added under ABI 106: no existing signature
 * changed. */
#define FR_CHIP_MAX_SIDE 4096
int fr_face_chips_u8(const uint8_t* frames, int N, int H, int W, const int32_t* chips, int F, int size, uint32_t bgr_fill,
                     uint8_t* out, fr_stream_t stream);
int fr_face_chips_refs_u8(const fr_frame_ref* refs, int nframes, const int32_t* chips, int F, int size, uint32_t bgr_fill,
                          uint8_t* out, fr_stream_t stream);

/* Device JPEG encoder: BGR u8 frames on the device (the drawn frames of the HUD) -> baseline JPEG files, so that a few hundred
 * KB per 1080p frame cross the link instead of 6.2 MB (the reference shows raw frames with cv2.imshow, one process per camera:
 * infrenceServer.py:648-667).  The bytes are DEFINED by tests/helpers/jpeg_ref.py and reproduced byte for byte (32-bit integer
 * arithmetic only): JFIF full-range YCbCr in libjpeg's 16-bit fixed point, the last column and row replicated
 * to multiples of 16, 4:2:0 chroma (a + b + c + d + 2) >> 2, MCUs of 16 x 16 (Y00 Y01 Y10 Y11 Cb Cr), libjpeg's integer
 * "islow" forward DCT of samples - 128, sign(c) ((|c| + (qv >> 1)) / qv) with qv = t << 3, the Huffman coding of T.81 F.1.2 with
 * the Annex K tables, ONE restart interval per MCU row (DRI = ceil(W / 16), DC predictions 0 at the start of a row, the last
 * byte of a row padded with 1-bits, 0x00 stuffed behind every 0xFF, RSTm with m = row mod 8 behind every row but the last).
 *
 * header: DEVICE bytes SOI .. SOS, FR_JPEG_HEADER_BYTES of them, built by the host once per quality (jpeg.py: APP0 JFIF 1.01,
 *   DQT 0 / 1, SOF0, four DHT, DRI, SOS); the H / W fields of SOF0 (FR_JPEG_AT_H, FR_JPEG_AT_W) and the interval of DRI
 *   (FR_JPEG_AT_DRI) are patched per frame here, so a ragged batch needs one header.
 * codes: DEVICE u32 [2][FR_JPEG_CODE_ROW], row 0 luma, row 1 chroma: entry s < 256 the AC code of symbol s (run << 4 | size),
 *   entry 256 + c the DC code of category c, each code << 8 | length (jpeg_tables.code_table; the library holds no copy).
 * qtables: DEVICE i32 [3][64]: the luma and the chroma quantisation table of the quality in natural order (1 .. 255), then the
 *   zigzag position of every natural index.
 * Two launches.  Rows: one workgroup per (frame, MCU row) codes the row into its segment of the workspace, row_budget bytes
 * long, and writes the row's byte length; every store is bounded by the budget.  Assemble: per frame the header, the rows back
 * to back with the RSTm markers between them and EOI are packed into `out`, the frames back to back: frame f is
 * out[offsets[f] .. offsets[f + 1]), offsets i64 [N + 1] with offsets[0] = 0.  status i32 [N]: FR_JPEG_OK; FR_JPEG_OVERFLOW - a
 * row of the frame did not fit row_budget, or the frame would end past out_capacity (then so would every frame behind it): the
 * frame has length 0, nothing of it is written, the other frames are untouched; FR_JPEG_SKIPPED (table form) - an entry with a
 * non-positive side, a side above 65535 or above max_H / max_W, of 2 GiB or more or with a null pointer: length 0 likewise.
 * Nothing is written past a row's budget, past out + out_capacity or past ws + ws_bytes.
 * workspace: fr_jpeg_workspace(N, H, W, row_budget) bytes, H x W the frames' size (the table form: max_H x max_W); 0 for
 * arguments the entries refuse.  A row of w pixels that is coded as it comes needs at most about 416 bytes per 8 x 8 block;
 * the host's default budget is the strip's raw BGR size, 16 * 16 ceil(w / 16) * 3.
 * Refused before any launch: N outside 0 .. 65535, H or W (max_H or max_W) outside 1 .. 65535, a frame of 2 GiB or more,
 * row_budget < 1, header_len != FR_JPEG_HEADER_BYTES, a negative out_capacity, a workspace that is too small, a null pointer with
 * N > 0.  N == 0 returns FR_OK and touches nothing.  Any byte alignment of the frames.  Added under ABI 106: no existing
 * signature changed. */
#define FR_JPEG_OK 0
#define FR_JPEG_OVERFLOW 1
#define FR_JPEG_SKIPPED 2
#define FR_JPEG_HEADER_BYTES 629
#define FR_JPEG_AT_H 163
#define FR_JPEG_AT_W 165
#define FR_JPEG_AT_DRI 613
#define FR_JPEG_CODE_ROW 272
size_t fr_jpeg_workspace(int N, int H, int W, int row_budget);
int fr_jpeg_encode_u8(const uint8_t* frames, int N, int H, int W, const uint8_t* header, int header_len, const uint32_t* codes,
                      const int32_t* qtables, int row_budget, uint8_t* out, int64_t out_capacity, int64_t* offsets,
                      int32_t* status, void* workspace, size_t workspace_bytes, fr_stream_t stream);
int fr_jpeg_encode_refs_u8(const fr_frame_ref* refs, int nframes, int max_H, int max_W, const uint8_t* header, int header_len,
                           const uint32_t* codes, const int32_t* qtables, int row_budget, uint8_t* out, int64_t out_capacity,
                           int64_t* offsets, int32_t* status, void* workspace, size_t workspace_bytes, fr_stream_t stream);

/* Device JPEG decoder: baseline JPEG files on the device (an MJPEG camera's frames, enrolment photos) -> BGR u8 frames, so
 * that the encoded bytes cross the link and the host never decodes (the reference decodes on the CPU: infrenceServer.py:573-601,
 * trainingServer.py:219-221).  The pixels are DEFINED by tests/helpers/jpeg_decode_ref.py and reproduced byte for byte (32-bit
 * integer arithmetic only); the definition is libjpeg's arithmetic: T.81 F.2.2 with the file's own tables,
 * coef * q, the "islow" inverse DCT, "fancy" chroma upsampling (replication for a component at most 2 samples wide), the 16-bit
 * fixed-point colour transform.  Baseline sequential, 8 bit, one interleaved scan, 3 components at 4:4:4 / 4:2:2 / 4:2:0 or 1
 * component, any restart interval or none.  The HOST parses SOI .. SOS (jpeg_decode.py) and never touches the entropy data.
 *
 * data: DEVICE bytes, the files (or only their scans) back to back, data_bytes of them.  frames: a DEVICE table, one entry per
 *   file: [scan_off, scan_off + scan_len) the entropy data - from behind SOS to the end of the file; the scan ends at the first
 *   marker that is no RSTm -, H x W, sampling FR_JPEGD_444 / _422 / _420 / _GRAY, restart the MCUs of a restart interval (0:
 *   none), and per component the tables: qsel an index into qtables, dcsel / acsel into htables.
 * qtables: DEVICE i32 [nq][64], natural order.  htables: DEVICE i32 [nh][FR_JPEGD_HUFF_ROW], one Huffman table each: [0, 512)
 *   the next 9 bits -> length << 8 | symbol (0: a longer code or none), [512, 530) maxcode by length (-1: no code of that
 *   length), [530, 548) valptr - mincode by length, [548, 804) HUFFVAL (jpeg_decode.huffman_row).  natural: DEVICE i32 [64],
 *   zigzag position -> natural index (jpeg_tables.ZIGZAG; the library holds no copy).
 * refs: a DEVICE frame table; entry f names the destination of file f, its H x W the file's.  status i32 [nframes]:
 *   FR_JPEGD_OK; FR_JPEGD_BAD_STREAM - the scan broke off, holds a code no table has, runs a coefficient index past 63, has a
 *   restart marker out of order or another number of intervals or blocks than the header implies: the frame's pixels are not
 *   written; FR_JPEGD_SKIPPED - an entry the launches cannot follow (a null destination, sizes that differ from the
 *   destination's or exceed max_H x max_W, an unknown sampling, a table index out of range, a scan outside data or of 2^28
 *   bytes and more, more restart intervals than max_segments): nothing of it is read or written.  The other frames are untouched
 *   either way, and no load or store leaves the scan, the workspace or the destination.
 * workspace: fr_jpeg_decode_workspace(nframes, max_H, max_W, max_segments) bytes on a 16-byte boundary (0 for arguments no
 *   decode exists for); max_segments: the most restart intervals any file has (1 without DRI).
 * Four launches on `stream`, no allocation, no synchronisation.  FR_E_INVALID before any launch for nframes outside 0 .. 65535,
 * max_H or max_W outside 1 .. 65535, max_H * max_W * 3 >= 2^31, max_segments outside 1 .. 2^24, nq or nh outside 1 .. 65535, a
 * negative data_bytes, a workspace that is too small or misaligned, a null pointer with nframes > 0.  nframes == 0 returns
 * FR_OK and touches nothing.  Added under ABI 106: no existing signature changed. */
#define FR_JPEGD_OK 0
#define FR_JPEGD_BAD_STREAM 1
#define FR_JPEGD_SKIPPED 2
#define FR_JPEGD_444 0
#define FR_JPEGD_422 1
#define FR_JPEGD_420 2
#define FR_JPEGD_GRAY 3
#define FR_JPEGD_HUFF_ROW 804
typedef struct {
    int64_t scan_off;
    int32_t scan_len;
    int32_t H, W, sampling, restart;
    int32_t qsel[3], dcsel[3], acsel[3];
} fr_jpeg_frame;
size_t fr_jpeg_decode_workspace(int nframes, int max_H, int max_W, int max_segments);
int fr_jpeg_decode_refs_u8(const uint8_t* data, int64_t data_bytes, const fr_jpeg_frame* frames, int nframes, int max_H, int max_W,
                           int max_segments, const int32_t* qtables, int nq, const int32_t* htables, int nh, const int32_t* natural,
                           const fr_frame_ref* refs, int32_t* status, void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* fr_jpeg_decode_refs_u8 with an EXIF orientation per frame (what cv2.imdecode applies for the reference's enrolment worker,
 * trainingServer.py:219-221).  orient: DEVICE i32 [nframes], 1 .. 8, defined by tests/helpers/orient_ref.py: 1 as coded, 2
 * mirrored left-right, 3 turned by 180 degrees, 4 mirrored top-bottom, 5 transposed, 6 turned clockwise, 7 transposed about the
 * other diagonal, 8 turned counter-clockwise; a null pointer means all 1 and IS fr_jpeg_decode_refs_u8, launch for launch.
 * refs entry f names the ORIENTED destination: H x W for 1 .. 4, W x H for 5 .. 8.  An orientation word outside 1 .. 8 or a
 * destination of the other shape is FR_JPEGD_SKIPPED.  frames, max_H, max_W and the workspace stay in CODED sizes.  The first
 * three launches are fr_jpeg_decode_refs_u8's; the last one writes every pixel once where its frame's orientation puts it, the
 * transposing ones through a tile in LDS so that stores run along destination rows.  Errors as fr_jpeg_decode_refs_u8.  Added
 * under ABI 106: no existing signature changed. */
int fr_jpeg_decode_oriented_refs_u8(const uint8_t* data, int64_t data_bytes, const fr_jpeg_frame* frames, int nframes, int max_H,
                                    int max_W, int max_segments, const int32_t* qtables, int nq, const int32_t* htables, int nh,
                                    const int32_t* natural, const fr_frame_ref* refs, const int32_t* orient, int32_t* status,
                                    void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* Behind fr_jpeg_decode_refs_u8, for destinations that are REUSED (a ring's device frames): zeroes the H * W * 3 bytes of every
 * frame whose status is FR_JPEGD_BAD_STREAM, so that a file whose scan broke off is a black frame and not the picture its
 * destination held before.  Frames with another status, and null or empty entries, are left alone.  One launch on `stream`, no
 * synchronisation.  FR_E_INVALID for nframes outside 0 .. 65535 or a null pointer with nframes > 0.  Added under ABI 106.
 * The workspace of fr_jpeg_decode_refs_u8 also holds, for whoever measures the entropy launch: in frame f's slot (slots of
 * fr_jpeg_decode_workspace(1, max_H, max_W, max_segments) bytes each), i32 [2 max_segments + k] the most rounds behind round 0
 * that any chunk of restart interval k needed. */
int fr_jpeg_blank_bad_refs_u8(const fr_frame_ref* refs, const int32_t* status, int nframes, fr_stream_t stream);

/* ---------------------------------------------------------------- face tracks ----
 * Between detect and align: is this detection a face the camera's previous frame already showed, so that the embedding held
 * for it can stand in for a new one?  (The reference embeds every face of every frame it keeps and sheds load by taking every
 * 2nd frame, peopleCount.py:938,962.)  Only the EMBEDDING is held, never an identity: the held row goes through the gallery
 * scan of the current call.  State lives on the device, per camera slot s < S with T <= 64 entries, and belongs to the caller
 * (zeroed once):
 *   tbox    f32 [S][T][4]        the box an entry was last seen at (x1, y1, x2, y2)
 *   tstate  i32 [S][T][4]        (live, since, misses, id): since = turns carried since the last embed, misses = turns unseen
 *   next_id i32 [S]              the id the slot's next new track gets
 *   bank    f32 [S][T][2][512]   (embedding, normed embedding) of the entry's last embed
 *
 * fr_track_associate_f32: boxes f32 [N][cap][4] and counts i32 [N] as the detectors leave them (descending score), slot i32 [N];
 * outputs entry, need, tid i32 [N][cap].  Frame i with s = slot[i], detections j = 0 .. counts[i] - 1 (clamped to 0 .. cap) one
 * after the other:
 *   o[t]    IoU of detection j and tbox[s][t] for every live entry, in float32 with one IEEE rounding per operation:
 *           area(b) = (b.x2 - b.x1 + 1) * (b.y2 - b.y1 + 1);  w = max(0, min(x2) - max(x1) + 1), h likewise, inter = w * h;
 *           o = inter / ((area(detection) + area(entry)) - inter)      (the form and operand order fr_sort_nms is pinned to);
 *           max / min pass a NaN on, so a NaN coordinate on either side gives o = NaN
 *   match   among the live entries not claimed this turn with o[t] >= iou_thr (false for a NaN): the largest o, the lowest t
 *           among equal values.  The entry is claimed, tbox[s][t] = the detection's box, misses = 0, entry = t, tid = id.
 *   carry   a matched detection with since < max_reuse and with NO other live entry of the slot, claimed or not, at o > 0:
 *           need = 0, since += 1.  Any other matched detection: need = 1, since = 0.  Faces that touch or cross are therefore
 *           always embedded again - the guard against handing one person's embedding to another.
 * then every live entry not claimed gets misses += 1 and live = 0 when misses > max_misses (nothing else of it changes); then
 * every unmatched detection, in j order, takes the lowest entry that is not live (those retired this turn included):
 * live = 1, since = misses = 0, id = next_id[s], next_id[s] += 1 (wrapping), tbox = its box, entry = t, tid = id, need = 1.  With no
 * such entry the detection stays untracked: entry = tid = -1, need = 1.  Slots j >= counts[i]: entry = -1, need = 0, tid = -1.
 * A frame whose slot is outside [0, S) has no state: need = 1, entry = tid = -1 for its detections, nothing else is touched.  Two
 * frames of one call must not name one slot (the result is then unspecified, every access still inside the arrays).
 * One launch on `stream`, one wave per frame with entry t in lane t, no synchronisation, allocation or atomics.
 * Refused before any launch: T or cap outside 1 .. 64, S < 1, N outside 0 .. 65535, negative max_reuse or max_misses, iou_thr
 * outside (0, 1] (a NaN included), a null pointer with N > 0.  N == 0 returns FR_OK and touches nothing.
 *
 * fr_track_commit_f32: after the embed net has filled the need = 1 rows of emb / normed f32 [N*cap][512] (slot layout), one
 * workgroup per (frame, detection slot j < counts) with 0 <= entry < T and a slot inside [0, S):
 *   need != 0:  bank[s][entry] = (emb row, normed row)          need == 0:  (emb row, normed row) = bank[s][entry]
 * as 16-byte moves; every other row of emb / normed and of bank is left untouched.  Refusals as above (those of its arguments).
 * Added under ABI 106: no existing signature changed. */
int fr_track_associate_f32(const float* boxes, const int32_t* counts, const int32_t* slot, int N, int cap, int S, int T,
                           float* tbox, int32_t* tstate, int32_t* next_id, float iou_thr, int max_reuse, int max_misses,
                           int32_t* entry, int32_t* need, int32_t* tid, fr_stream_t stream);
int fr_track_commit_f32(const int32_t* entry, const int32_t* need, const int32_t* slot, const int32_t* counts, int N, int cap,
                        int S, int T, float* bank, float* emb, float* normed, fr_stream_t stream);

/* fr_track_resolve_quality_i32: the judging tracks' decision, between fr_face_quality_f16 and the one host copy of a turn.  The
 * bank then holds a track's last FIT embedding, and a face that turns unfit for a few frames keeps the row (and so whatever
 * identity the current call's scan gives that row).  State beside tstate, the caller's, zeroed once:
 *   tqual   i32 [S][T][4]        (has, age, id, 0): age = turns the held row has stood in since it was embedded
 * Entry t of slot s HOLDS A FIT ROW FOR THE CURRENT TRACK iff has == 1 and tqual.id == tstate.id.  A retired entry taken by a new
 * track, a slot given back and taken again, and tracks dropped after a failed embed pass all end in a track with a fresh id
 * from next_id, so the id comparison alone keeps an entry from answering with the previous person's row: nothing zeroes tqual.
 * Inputs i32 [N][cap]: entry, need, tid as fr_track_associate_f32 wrote them THIS turn, verdict as fr_face_quality_f16 wrote it
 * (0: fit); slot, counts i32 [N] (counts clamped to 0 .. cap).  Per detection slot (i, j) with j < counts[i], s = slot[i]:
 *   A. entry outside [0, T) (untracked) or s outside [0, S) (stateless):  action = EMBED if verdict == 0 else REJECT; no state
 *      is touched.
 *   B. otherwise, valid = holds a fit row for tid:
 *        need == 0 and valid and age < max_age:  CARRY,  age += 1; tstate stays as the associate launch wrote it
 *        else verdict == 0:                      EMBED,  tqual = (1, 0, tid, 0), tstate.since = 0
 *        else:                                   REJECT, tstate.since = 0; valid and age < max_age: age += 1 (the row stays for
 *                                                a later carry), else has = 0
 * Outputs i32 [N][cap], EVERY slot written: action (0 no face, 1 EMBED, 2 CARRY, 3 REJECT) and need2 / entry2 for
 * fr_track_commit_f32: EMBED (1, entry), CARRY (0, entry), REJECT and no face (0, -1) - commit then touches neither the bank nor
 * the row.  A face the associate launch wants embedded (need == 1) is never given a held row in the same turn: the crossing
 * guard stays exactly the associate launch's.  A blurred face of a crowded frame is REJECT; a blurred face standing alone is
 * rejected on the turn its re-embed is due and carried from the next while age < max_age.
 * One launch on `stream`, one thread per detection slot, plain vector stores; no atomics, LDS, allocation or synchronisation:
 * each (slot, entry) is claimed by at most one detection per turn and a call must not name a slot twice, so no two threads
 * touch one tqual / tstate row.  Refused before any launch: T or cap outside 1 .. 64, S < 1, N outside 0 .. 65535, max_age < 0,
 * a null pointer with N > 0.  N == 0 returns FR_OK and touches nothing.  Added under ABI 106: no existing signature changed. */
int fr_track_resolve_quality_i32(const int32_t* entry, const int32_t* need, const int32_t* tid, const int32_t* verdict,
                                 const int32_t* slot, const int32_t* counts, int N, int cap, int S, int T, int32_t* tstate,
                                 int32_t* tqual, int max_age, int32_t* action, int32_t* need2, int32_t* entry2,
                                 fr_stream_t stream);

/* fr_track_fuse_f32: track templates, behind fr_track_commit_f32.  An entry keeps the unit embeddings of its track's last K shots
 * and their unit mean, and that mean - not this frame's row alone - is what the gallery scan is asked with.  (The reference has
 * this rule for unknown people only: UnknownPerson keeps a 10-deep ring and compares against its mean, peopleCount.py:63-79.)
 * A shot joins a template only if it agrees with it; otherwise the template starts over from that shot alone, so a shot that
 * fails the test is answered with the very bits the embed net gave.  State beside the bank, the caller's, zeroed once, K in 1 .. 16:
 *   tring   f32 [S][T][K][512]   the unit (normed) embeddings of the entry's last shots
 *   ttmpl   i32 [S][T][4]        (len, head, id, 0)
 *   tmean   f32 [S][T][512]      the template, a unit row
 * Entry t of slot s HOLDS A TEMPLATE FOR TRACK id iff len >= 1 and ttmpl.id == id; as with tqual, the id comparison alone covers a
 * slot given back, dropped tracks and a retired entry taken by a new track: nothing zeroes this state.
 * Inputs: entry, need i32 [N][cap] as fr_track_commit_f32 got them this turn (under judging tracks entry2 / need2), tid of the
 * associate launch, slot, counts i32 [N] (clamped to 0 .. cap), normed f32 [N*cap][512] after the commit launch.  Per detection
 * slot q = (i, j) with j < counts[i], s = slot[i] inside [0, S) and e = entry[q] inside [0, T), n = row q of normed:
 *   need != 0 (embedded this turn):
 *     the entry holds a template for tid[q]:  c = dot(n, tmean[s][e]), lane l of a wave taking floats 8l .. 8l+7: eight rounded
 *         products summed left to right, then the xor-shuffle sum over offsets 32 .. 1 (the dot of fr_gallery_first_above_f32)
 *       c >= join_thr:                JOINED     ring[head] = n, head = (head + 1) % K, len = min(len + 1, K)
 *       else (a NaN included):        RESTARTED  ring[0] = n, head = 1 % K, len = 1
 *     it does not hold one:           STARTED    as RESTARTED, and ttmpl.id = tid[q]
 *     then tmean[s][e] = n's bits when len == 1 (no arithmetic), otherwise the ring rows OLDEST FIRST (from head when len == K,
 *     else from 0) summed in that order from 0.f, divided by (float)len (fr_mean_rows_f32), then v / ||v|| in the arithmetic of
 *     fr_l2norm_rows_f32;  query[q] = tmean[s][e], shots[q] = len
 *   need == 0 (carried):
 *     the entry holds a template for tid[q]:  READ  query[q] = tmean[s][e], shots[q] = len; no state moves
 *     otherwise:                                    query[q] = n, shots[q] = 0, event NONE
 * Every other slot (untracked, stateless, rejected, past the count): query[q] = normed[q], shots[q] = 0, event NONE.  Every row
 * of query f32 [N*cap][512], shots and event i32 [N][cap] is written (0 NONE, 1 STARTED, 2 JOINED, 3 RESTARTED, 4 READ); no other
 * row of the state is touched.  With K = 1 the template is the last embedded row: query == normed bit for bit.  State this rule
 * did not write at this K (len > K, head outside [0, K)) gives an unspecified template, every access still inside the arrays.
 * One launch on `stream`, one wave per (frame, detection slot), plain vector loads and stores; no atomics, LDS, allocation or
 * synchronisation: each (slot, entry) is claimed by at most one detection per turn and a call must not name a slot twice.  The
 * row written this turn is never read back from memory.  Refused before any launch: T or cap outside 1 .. 64, S < 1, N outside
 * 0 .. 65535, K outside 1 .. 16, join_thr outside [-1, 1] (a NaN included), a null pointer with N > 0.  N == 0 returns FR_OK and
 * touches nothing.  Added under ABI 106: no existing signature changed. */
int fr_track_fuse_f32(const int32_t* entry, const int32_t* need, const int32_t* tid, const int32_t* slot, const int32_t* counts,
                      const float* normed, int N, int cap, int S, int T, int K, float join_thr, float* tring, int32_t* ttmpl,
                      float* tmean, float* query, int32_t* shots, int32_t* event, fr_stream_t stream);

/* ---------------------------------------------------------------- face quality ----
 * Between align and embed: is this aligned face worth the embed net and a gallery scan?  (The reference embeds every detected
 * face, infrenceServer.py:528-532; its only guard is the silent [0.35, 0.45) drop band of the counting path.)  The crops are in
 * fixed geometry, so what is measured on them compares between faces of any size in the frame.
 *   crops        f16 [S][112][112][8] as fr_warp_affine_5pt* write them: channels 0..2 are R, G, B as (u - 127.5) / 127.5
 *   kps          f32 [S][5][2] in frame pixels: left eye, right eye, nose, left mouth, right mouth
 *   slot_counts  i32 [S / cap] with cap: slot s holds a face iff s % cap < slot_counts[s / cap];  NULL: all S rows hold faces
 *   qi i32 [S][8], qf f32 [S][4], verdict i32 [S]      the outputs
 * A slot without a face writes verdict = -1 and zeros, and reads neither its crop nor its kps.
 * Pixel: per channel u = rint(h * 127.5f + 127.5f) clamped to 0 .. 255, two singly rounded f32 operations (the byte the warp
 * rounded to, for all 256 values);  L = (77 R + 150 G + 29 B + 128) >> 8, the activity gate's weights.
 * Window: rows 20 .. 99 and columns 16 .. 95 inclusive, n = 6400 pixels, the face interior of the ArcFace template; the Laplacian
 * also reads the one-pixel ring round it (rows 19 .. 100, columns 15 .. 96).  Nothing else of the crop is read.
 * Integer metrics, exact (the same bytes from any launch shape), over the window:
 *   D(y,x) = 4 L(y,x) - L(y-1,x) - L(y+1,x) - L(y,x-1) - L(y,x+1)
 *   qi[0] = mean     = (sum L + n/2) / n
 *   qi[1] = contrast = (n sum L^2 - (sum L)^2) / n^2        64-bit, floor
 *   qi[2] = sharp    = (n sum D^2 - (sum D)^2) / n^2        64-bit, floor; sum D^2 reaches 6 658 560 000 on a checkerboard (more
 *                                                           than 2^32), sharp itself is at most 1 040 400
 *   qi[3] = dark   = pixels with L <= 15        qi[4] = bright = pixels with L >= 240        qi[5..7] = 0
 * Landmark metrics, float32, one IEEE rounding per operation in exactly this order (no fused multiply-add, no division):
 *   e = re - le;  d2 = e.x e.x + e.y e.y;  a = nose - le;  t = a.x e.x + a.y e.y;  mid = (lm + rm) 0.5f;
 *   c = cross(e, a);  m = cross(e, mid - le)  with cross(a, b) = a.x b.y - a.y b.x;      qf = (d2, t, c, m)
 * (on the template itself t / d2 = 0.500 and c / m = 0.495).
 * Verdict: 0 when the face is fit, otherwise the sum of
 *     1 small    d2 < min_eye2                 2 dark     mean < mean_lo             4 bright  mean > mean_hi
 *     8 flat     contrast < contrast_min      16 blurred  sharp < sharp_min         32 clipped dark + bright > clip_max
 *    64 yaw      fabsf((t + t) - d2) > yaw_max d2
 *   128 pitch    !(m > 0), or c < pitch_lo m, or c > pitch_hi m
 * One launch on `stream`, one workgroup per slot, no allocation, atomics or synchronisation.  Refused before any launch: S
 * outside 0 .. 65535 * 64, cap < 1 with slot_counts given, min_eye2 negative, infinite or NaN, mean_lo or mean_hi outside
 * 0 .. 255, negative contrast_min or sharp_min, clip_max outside 0 .. 6400, yaw_max negative or NaN (infinity switches the
 * test off), pitch_lo > pitch_hi or a NaN among them (infinities allowed), and with S > 0 a null crops, kps, qi, qf or verdict or
 * crops not on a 16-byte boundary.  S == 0 returns FR_OK and touches nothing.  Added under ABI 106: no existing signature changed. */
int fr_face_quality_f16(const void* crops, const float* kps, const int32_t* slot_counts, int cap, int S, int32_t* qi, float* qf,
                        int32_t* verdict, float min_eye2, int mean_lo, int mean_hi, int contrast_min, int sharp_min, int clip_max,
                        float yaw_max, float pitch_lo, float pitch_hi, fr_stream_t stream);

/* ---------------------------------------------------------------- SCRFD detector ----
 * The detector of insightface's buffalo_l pack (det_10g.onnx; FaceAnalysis(name="buffalo_l"), infrenceServer.py:412-416) as
 * layer kernels; the host walks a plan read from the ONNX graph (onnx_import.scrfd_plan_from_onnx, scrfd.py).  Activations are
 * f16 NHWC with the channel count padded to a multiple of 8; padded channels hold exact zeros.
 *
 * fr_det_conv_f16: y = [relu]( conv(x, w) + bias [+ residual] ), 1x1 or 3x3, stride 1 or 2, zero padding `pad` on every side,
 * f16 operands on the matrix cores, f32 accumulation and epilogue (bias, then residual, then ReLU).
 *   x         f16 [N,H,W,Cin], Cin a multiple of 8
 *   w         f16, fr_det_conv_weight_halves(Cin, cout_packed, K) elements: [ceil(G / 4)][cout_packed][4][8] where G = K*K*Cin/8
 *             and element [s][co][q][j] is weight (co, tap t, channel 8*c + j) of group g = 4 s + q = t * (Cin / 8) + c, tap
 *             t = ky * K + kx; groups >= G and output channels past the layer's own are zero.  cout_packed: a multiple of 16.
 *   bias      f32 [cout_packed] (zero past the layer's own channels)
 *   residual  optional f16 [N,Ho,Wo,ldo] (f16 output only)
 *   y         out_f32 == 0: f16 [N,Ho,Wo,ldo], channels [0, cout_store) written, cout_store and ldo multiples of 8;
 *             out_f32 != 0: f32 [N,Ho,Wo,ldo], channels [0, cout_store) written, any cout_store <= ldo (the head maps)
 *   tile      0: chosen from the shape; else 10 * MT + NT with MT in {1, 2, 4} (x16 pixels per wave), NT in {2, 4} (x16 channels) */
size_t fr_det_conv_weight_halves(int Cin, int cout_packed, int K);
int fr_det_conv_f16(const void* x, const void* w, const float* bias, const void* residual, void* y, int N, int H, int W,
                    int Cin, int cout_packed, int K, int stride, int pad, int Ho, int Wo, int cout_store, int ldo,
                    int relu, int out_f32, int tile, fr_stream_t stream);
/* fr_det_conv_act_f16: fr_det_conv_f16 with a choice of activation - y = act( conv(x, w) + bias [+ residual] ), the epilogue in
 * that order.  Operands, packing, outputs and `tile` as above.  The layers of a MobileFaceNet recogniser that are no depthwise
 * convs: the 3x3 stride-2 stem on the 8-channel aligned crop and the 1x1 expand convs (PReLU), the 1x1 project convs (linear,
 * with the block's input as residual) and the final fully connected layer as a 1x1 conv on a 1x1 map (out_f32).
 *   act       0: none, 1: ReLU (the bits of fr_det_conv_f16 with relu = 1), 2: PReLU v < 0 ? v * slope[channel] : v
 *   slope     f32 [cout_packed], read only when act == 2 (values past the layer's own channels are never stored) */
int fr_det_conv_act_f16(const void* x, const void* w, const float* bias, const float* slope, const void* residual, void* y,
                        int N, int H, int W, int Cin, int cout_packed, int K, int stride, int pad, int Ho, int Wo,
                        int cout_store, int ldo, int act, int out_f32, int tile, fr_stream_t stream);
/* Depthwise convolution: y[n,oy,ox,c] = act( sum over the in-bounds taps (ky, kx) of x[n, oy*stride - pad + ky, ox*stride - pad
 * + kx, c] * w[ky*K + kx][c] + bias[c] ).  The layer MobileFaceNet (w600k_mbf.onnx) and the small SCRFD detectors (det_500m.onnx)
 * are built from; memory-bound, no matrix-core work.
 *   x         f16 [N,H,W,C], C a multiple of 8 (fr_det_conv_f16's activation layout; padded channels hold zeros)
 *   w         f16 [K*K][C], tap-major: the 8 channels a lane owns are one 16-byte load per tap
 *   bias      f32 [C]
 *   slope     f32 [C], read only when act == 2
 *   y         f16 [N,Ho,Wo,C]; Ho = (H + 2 pad - K) / stride + 1 and Wo likewise, computed by the host and checked here
 *   K         odd, <= 7; stride 1 or 2; pad 0 .. K / 2, zero padding: taps outside the input are skipped
 *   act       0: none, 1: ReLU, 2: PReLU
 * f32 accumulation over the taps in (ky, kx) order (a product of two f16 is exact in f32), + bias, activation, ONE rounding to
 * f16.  An element's bits depend on neither N, the image's position in the batch nor the launch's tiling.  K == H == W with pad 0
 * (one output pixel per image and channel: MobileFaceNet's 7x7 tail) walks the taps from global memory; every other shape
 * stages the input rows of a band of output rows in LDS, so each input element is fetched about once. */
int fr_dw_conv_f16(const void* x, const void* w, const float* bias, const float* slope, void* y, int N, int H, int W, int C, int K,
                   int stride, int pad, int Ho, int Wo, int act, fr_stream_t stream);
/* canvas u8 [N,H,W,3] BGR -> y f16 [N,H,W,8]: channels 0..2 = (R, G, B) as (v - 127.5) / 128 (exact in f16), 3..7 = 0
 * (insightface's SCRFD blob: input_mean = 127.5, input_std = 128, swapRB). */
int fr_det_input_f16(const uint8_t* canvas, void* y, int N, int H, int W, fr_stream_t stream);
/* x f16 [N,H,W,C] -> y f16 [N,Ho,Wo,C], C a multiple of 8.  kind 0: max, 1: average; window k <= 3, stride <= 2, `pad` rows /
 * columns in front; Ho, Wo from the host (floor or ceil mode): every window must hold an in-bounds tap.  Taps outside the
 * input are skipped and the average divides by the in-bounds count (ONNX count_include_pad = 0; with no window over padding
 * or the edge, which is all the importer admits of count_include_pad = 1, the two agree).  Exact: the f16 rounding of the
 * true value. */
int fr_det_pool_f16(const void* x, void* y, int N, int H, int W, int C, int Ho, int Wo, int kind, int k, int stride,
                    int pad, fr_stream_t stream);
/* y = lateral + nearest-neighbour x`up` of coarse (up = 2: the FPN top-down step; 1: a plain sum).  lateral, y f16 [N,H,W,C];
 * coarse f16 [N,H/up,W/up,C]; C a multiple of 8.  One f16 rounding of the exact sum. */
int fr_det_upsample_add_f16(const void* coarse, const void* lateral, void* y, int N, int H, int W, int C, int up,
                            fr_stream_t stream);
/* One level of SCRFD head maps -> candidates.  score f32 [nframes,Hl*Wl*A] (LOGITS), bbox f32 [nframes,Hl*Wl*A,4], kps f32
 * [nframes,Hl*Wl*A,10], anchors of a cell consecutive, cells row-major.  Keeps anchors with logit >= logit_thr in that order,
 * the first `cap`; anchor centre (x * stride, y * stride); box = (cx - d0 s, cy - d1 s, cx + d2 s, cy + d3 s), keypoint i =
 * (cx + k[2i] s, cy + k[2i+1] s), all divided by det_scale[frame] (f32 [nframes]); score = 1 / (1 + expf(-logit)).  Each
 * operation is one IEEE f32 rounding.  Writes segment `level` (0..2) of boxes f32 [nframes,3,cap,4], scores f32 [nframes,3,cap],
 * aux f32 [nframes,3,cap,10] and counts i32 [nframes*3]: the lists fr_sort_nms takes with nseg = 3, seg_cap = cap. */
int fr_scrfd_decode(const float* score, const float* bbox, const float* kps, int nframes, int Hl, int Wl, int A, int stride,
                    int level, float logit_thr, const float* det_scale, int cap, float* boxes, float* scores, float* aux,
                    int32_t* counts, fr_stream_t stream);

/* A recorded run of detector calls replayed by ONE C call (an eager single-frame get() is bound by the interpreter: ~50
 * ctypes calls per frame; FaceAnalysis.get, infrenceServer.py:528).  `fn` names the entry point, `a` carries its arguments
 * as 8-byte slots in declaration order: pointers and size_t as they are, ints sign-extended, floats as their IEEE bits in
 * the low word.  Two further ids record / wait for an event of the CALLER's (no allocation here): a recorded call may deal
 * the pyramid levels over side streams.  Same kernels, same order per stream, same bits as the individual calls; stops at
 * the first failing call.  `nargs` must be the entry point's arity (18 / 21 / 16 / 18 / 8 / 13 / 14, 2 for the event ids):
 * a short or malformed entry is refused before anything is launched. */
enum { FR_FN_DCONV_MFMA = 1, FR_FN_PNET23 = 2, FR_FN_PNET_CANDIDATES = 3, FR_FN_SORT_NMS = 4, FR_FN_BOX_REFINE = 5,
       FR_FN_CROP_CONV1 = 6, FR_FN_STAGE_SELECT = 7,
       FR_FN_EVENT_RECORD = 8 /* a = (hipEvent_t, hipStream_t) */, FR_FN_STREAM_WAIT = 9 /* a = (hipStream_t, hipEvent_t) */ };
typedef struct {
    int32_t fn; int32_t nargs;
    uint64_t a[22];
} fr_call;
int fr_detect_sequence(const fr_call* calls, int ncalls);

#ifdef __cplusplus
}
#endif
#endif
