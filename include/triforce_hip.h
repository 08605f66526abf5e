/*
 * triforce_hip.h — C ABI of libtriforce_hip.so (hand-written gfx950 / CDNA4 kernels for the
 * TriForce hierarchical draft/verify decode path).
 *
 * The reference (Infini-AI-Lab/TriForce @ 2024-10-08) has no FFI layer: its native boundary is
 * the third-party op flash_attn.flash_attn_with_kvcache plus torch kernels called from Python
 * (SURVEY.md §8b, B4).  Each entry point below replaces one such native call site; the citation
 * on every declaration is the reference file:line it stands in for.  INTEGRATION.md shows the
 * ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - fp16 tensors are passed as `const void*` / `void*` (IEEE binary16, last dim contiguous);
 *   - KV caches are addressed as base + token*stride_t + head*stride_h + d  (strides in ELEMENTS),
 *     so both the reference layout [T][H][D] and the head-major layout [H][T][D] used by
 *     triforce_amd are valid inputs;
 *   - every function enqueues work on `stream` (a hipStream_t passed as void*), allocates nothing,
 *     never synchronises and is hipGraph-capturable; workspaces are caller-provided;
 *   - return value: 0 on success, a negative errno-style code on bad arguments (TF_E*), or the
 *     positive hipError_t of a failed launch.
 *
 * ROUNDING OF fp16(a * b).  Wherever a contract below writes fp16(a * b) with an fp32 operand — the
 * normalisation fp16(x * inv) of every RMSNorm, the FP8 row scale fp16(s[n] * acc), the chunk mean
 * fp16(sum * (1 / chunk)) — the product is rounded to fp32 and THAT value to fp16: two roundings, as
 * torch and the reference compute it.  One rounding of the exact product (what a fused multiply-convert
 * instruction gives) differs by one fp16 spacing wherever the fp32 product lands on an fp16 midpoint;
 * tests/test_gpu_rounding_probes.py holds every such site to the two roundings on inputs where the
 * two differ.  (A product of two fp16 values is exact in fp32: there the question does not arise.)
 */
#ifndef TRIFORCE_HIP_H
#define TRIFORCE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TF_OK        0
#define TF_EINVAL  (-22)   /* bad argument (shape / alignment / unsupported head_dim)        */
#define TF_ENOSPC  (-28)   /* caller-provided workspace too small                           */
#define TF_ERANGE  (-34)   /* size exceeds what the kernel supports (e.g. chunks > 32768)    */

/* ABI version; bumped on any signature change. */
int tf_abi_version(void);

/* -------------------------------------------------------------------------------------------
 * Verify / decode attention  (replaces flash_attn_with_kvcache(q, k_cache, v_cache,
 * softmax_scale, causal=True): models/modeling_llama.py:240, models/tensor_op.py:168,316)
 *
 * Split-KV attention of sq <= 32 query rows against sk cached keys per head, bottom-right
 * aligned causal mask (query i sees keys [0, sk - sq + i]).  QK^T and PV run on MFMA
 * (v_mfma_f32_16x16x32_f16 / 16x16x16_f16), softmax in fp32, output fp16.
 *   q        [sq][H][D] fp16 (post-RoPE)
 *   k, v     layer base of the cache, see stride convention above; keys [0, sk) are read
 *   out      [sq][H*D] fp16
 *   sk_dev   optional device int32: if non-NULL the key count is read from it at run time (lets a
 *            captured hipGraph follow a growing cache); `sk` is then the upper bound used to size
 *            the launch
 *   ws       float workspace, at least tf_attn_decode_ws_floats(H, sq, D, nsplit) floats
 *   nsplit   number of KV splits per head (>=1); tf_attn_decode_pick_nsplit gives a default
 * D must be 64 or 128.
 * ------------------------------------------------------------------------------------------- */
int64_t tf_attn_decode_ws_floats(int H, int sq, int D, int nsplit);
int tf_attn_decode_pick_nsplit(int H, int sk);
int tf_attn_decode(const void* q, const void* k, const void* v, void* out,
                   int64_t stride_t, int64_t stride_h,
                   int sq, int sk, const int32_t* sk_dev, int H, int D, float scale,
                   int nsplit, float* ws, int64_t ws_floats, void* stream);
/* The same call as ONE launch (tf_attn_decode is split kernel + merge kernel): the last workgroup of each head to
 * finish merges that head's splits inside the split kernel — same arithmetic in the same order, bit-identical output.
 *   tickets  H uint32 words of device memory, ZERO before the first call; every call leaves them zero.  One ticket
 *            array serves one stream: calls that may run concurrently need separate arrays.
 * Falls back to the two-launch form when 3 * nsplit * 16*ceil(sq/16) floats do not fit the kernel's 64*(D+1)-float
 * merge scratch (e.g. D = 128: nsplit > 172 at sq <= 16). */
int tf_attn_decode_fused(const void* q, const void* k, const void* v, void* out,
                         int64_t stride_t, int64_t stride_h,
                         int sq, int sk, const int32_t* sk_dev, int H, int D, float scale,
                         int nsplit, float* ws, int64_t ws_floats, uint32_t* tickets, void* stream);
/* tf_attn_decode / tf_attn_decode_fused (tickets != NULL) with the OUTPUT in an explicit activation layout: element (row,
 * column c = h * D + d) at out[row * out_sm + (c / 8) * out_sk + c % 8] (see tf_skinny_gemm_act; row-major = H * D, 8). */
int tf_attn_decode_act(const void* q, const void* k, const void* v, void* out, int64_t out_sm, int64_t out_sk,
                       int64_t stride_t, int64_t stride_h, int sq, int sk, const int32_t* sk_dev, int H, int D,
                       float scale, int nsplit, float* ws, int64_t ws_floats, uint32_t* tickets, void* stream);
/* tf_attn_tune(0, v): v = 0 (default) keeps the split merge of > 8 splits as a second launch; 1 lets small grids (H * nsplit
 * <= 256, H <= 64, D = 128) merge inside the launch by a rendezvous of the head's workgroups (csrc/attn.hip; measured
 * slower, profiles/r04_attn_rendezvous_merge_ab.jsonl).  Returns the previous value, -1 for an unknown key.  Bit-identical
 * either way. */
int tf_attn_tune(int key, int value);

/* -------------------------------------------------------------------------------------------
 * Block attention: 1 <= sq <= 128 query rows in ONE pass over the keys.
 *   mask == NULL  bottom-right causal — flash_attn_with_kvcache with q_len = 128 in the chunked prefill
 *                 (utils/graph_infer.py:30-37 -> models/modeling_llama.py:240; models/TP_llama.py:246-250 ->
 *                 models/tensor_op.py:168).
 *   mask != NULL  tree attention — F.scaled_dot_product_attention with the dense additive [prefix | tree] mask
 *                 of the Sequoia path (models/tensor_op.py:171,265; masks built at utils/SpecTree_TP.py:65-67,
 *                 83-87,170): keys [0, tree_start) are visible to every row, key tree_start + j is visible to
 *                 query row i iff bit (j % 32) of mask[(mask_row0 + i) * mask_words + j / 32] is set; keys
 *                 [tree_start, sk) must fit 32 * mask_words bits.
 * Each workgroup's waves own 32 query rows apiece and walk the same key tiles, so the KV cache is streamed
 * from HBM once per call.  ws: at least tf_attn_block_ws_floats(H, D, nsplit) floats.
 * ------------------------------------------------------------------------------------------- */
int64_t tf_attn_block_ws_floats(int H, int D, int nsplit);
int tf_attn_block_pick_nsplit(int H, int sq, int sk);
int tf_attn_block(const void* q, const void* k, const void* v, void* out,
                  int64_t stride_t, int64_t stride_h, int sq, int sk, int H, int D, float scale,
                  int nsplit, float* ws, int64_t ws_floats,
                  const uint32_t* mask, int mask_words, int mask_row0, int tree_start, void* stream);

/* Whole-chunk causal prefill: 1 <= sq <= 4096 query rows (bottom-right aligned: row i sees keys [0, sk - sq + i]) in
 * ONE launch — the chunked prefill's attention (utils/graph_infer.py:30-37 -> models/modeling_llama.py:240 with
 * q_len = the chunk).  The 128-row blocks of the chunk that read the same key range run together on one XCD and share
 * its L2, so the KV cache is streamed from HBM about once per chunk instead of once per 128 rows.
 * (H * nsplit) % 8 must be 0 (tf_attn_prefill_pick_nsplit returns such a value); sk >= sq. */
int tf_attn_prefill_pick_nsplit(int H, int sq, int sk);
int64_t tf_attn_prefill_ws_floats(int H, int sq, int D, int nsplit);
int tf_attn_prefill(const void* q, const void* k, const void* v, void* out,
                    int64_t stride_t, int64_t stride_h, int sq, int sk, int H, int D, float scale,
                    int nsplit, float* ws, int64_t ws_floats, void* stream);

/* -------------------------------------------------------------------------------------------
 * Draft (Llama-68M) attention with RoPE applied to the cached keys on read
 * (models/modeling_llama_68m.py:151-190): keys are cached UN-rotated and rotated with
 * cache-relative positions 0..kv_len-1 at every call; q arrives already rotated.
 *   q [sq][H][D] fp16, k/v cache rows [0,kv_len), cos/sin [max_pos][D] fp16, out [sq][H*D].
 * D must be 64.  Bottom-right causal.
 * ------------------------------------------------------------------------------------------- */
int tf_attn_rope_on_read(const void* q, const void* k, const void* v, const void* cos, const void* sin,
                         void* out, int64_t stride_t, int64_t stride_h,
                         int sq, int kv_len, int H, int D, float scale, void* stream);

/* -------------------------------------------------------------------------------------------
 * The Llama-68M draft forward as one entry point (models/modeling_llama_68m.py:129-190 with the StreamingLLM cache of
 * models/cache.py:266-330; utils/graph_infer.py:52-57 `draft_run`): n <= 32 token ids -> fp32 logits [n][vocab] and,
 * when probs_out != NULL, softmax(top_p(logits[n-1] / temperature)) [vocab] (utils/sampling.py:43-60).
 * Native host code: the call issues the whole launch chain (embedding + positions, per layer RMSNorm + q|k|v + RoPE +
 * KV append / rope-on-read attention / o_proj + residual / RMSNorm + gate|up + SwiGLU / down_proj + residual, final
 * RMSNorm + lm_head, top-p) on `stream` through the kernels of the entry points above — bit-identical to calling them
 * one by one — allocates nothing and is graph-capturable.
 *   model  device pointers: embed [vocab][hidden] fp16; per layer ln1 / ln2 [hidden], wqkv packed in ROTARY-PAIR row
 *          order (tf_skinny_qkv_rope), wo / wgate / wup / wdown packed (tf_skinny_gemm); norm, lm_head packed;
 *          cos / sin [max_pos][head_dim] fp16.  head_dim must be 64 (tf_attn_rope_on_read).
 *   cache  per layer K / V base pointers, stride convention of the top of this file; keys are stored UN-rotated
 *   slot0  cache row of ids[0] (the rows [slot0, slot0 + n) are written); kv_len >= slot0 + n keys are attended
 *   ws     >= tf_draft_forward_ws_bytes(model, n) bytes of device scratch
 * ------------------------------------------------------------------------------------------- */
#define TF_DRAFT_MAX_LAYERS 8
typedef struct TfDraftModel {
    const void* embed;
    const void* ln1[TF_DRAFT_MAX_LAYERS];
    const void* wqkv[TF_DRAFT_MAX_LAYERS];
    const void* wo[TF_DRAFT_MAX_LAYERS];
    const void* ln2[TF_DRAFT_MAX_LAYERS];
    const void* wgate[TF_DRAFT_MAX_LAYERS];
    const void* wup[TF_DRAFT_MAX_LAYERS];
    const void* wdown[TF_DRAFT_MAX_LAYERS];
    const void* norm;
    const void* lm_head;
    const void* cos;
    const void* sin;
    int32_t layers, hidden, heads, head_dim, inter, vocab;
    float eps, scale;
} TfDraftModel;
typedef struct TfDraftCache {
    void* k[TF_DRAFT_MAX_LAYERS];
    void* v[TF_DRAFT_MAX_LAYERS];
    int64_t stride_t, stride_h;
} TfDraftCache;
int64_t tf_draft_forward_ws_bytes(const TfDraftModel* model, int n);
int tf_draft_forward_68m(const TfDraftModel* model, const TfDraftCache* cache, const int64_t* ids, int n, int slot0,
                         int kv_len, float* logits_out, float* probs_out, float temperature, float top_p,
                         void* ws, int64_t ws_bytes, void* stream);

/* The same forward as ONE LAUNCH (csrc/draft_persist.hip; replaces the ~40 kernels of models/modeling_llama_68m.py:129-190
 * + utils/sampling.py:5-27,43-60 per draft step, and the 13 launches of tf_draft_forward_68m): 256 co-resident workgroups,
 * the stages meet through per-edge arrival counters in `ctl` (write-through stores, agent-scope loads, no fences, no
 * cooperative launch).  Outputs — logits, the probability row, the K / V rows written — are BIT-IDENTICAL to
 * tf_draft_forward_68m.  Shapes: hidden 768, 12 heads of 64, inter 3072, 1-2 layers, vocab % 16 == 0 and <= 32768,
 * 1 <= n <= 16, kv_len <= 384, a device with >= 256 compute units (tf_draft_persist_supported: 0 = taken, TF_EINVAL /
 * TF_ERANGE otherwise — the caller keeps tf_draft_forward_68m).
 *   ws    >= tf_draft_persist_ws_bytes(model) bytes of device scratch, 256-byte aligned, owned by this control block's launches
 *   ctl   tf_draft_persist_ctl_bytes() bytes of device memory, 64-byte aligned, ZERO-filled once (tf_draft_persist_reset);
 *         launches on one ctl must be stream-ordered (graph replays of one engine are).
 * Every wait is bounded by wall-clock time (tf_draft_persist_tune key 0, ms, default 2000; frozen into captured graphs).
 * A time-out sets the sticky error word of ctl (+ the optional pinned host mirror): the outputs of that and of every later
 * launch are NaN until tf_draft_persist_reset.  tf_draft_persist_error: 0 or 1 + index of the edge whose wait timed out
 * (blocking read).  tf_draft_persist_tune key 1 = fault injection for tests (edge index + 1 whose first producer loses its
 * arrival; 0 off).  tf_draft_persist_stamps: device buffer of 256 x (return value) u64 100-MHz wall-clock stamps per
 * workgroup written by the following launches (NULL: off) — tools/draft_persist_stamps.py. */
int64_t tf_draft_persist_ctl_bytes(void);
int64_t tf_draft_persist_ws_bytes(const TfDraftModel* model);
int tf_draft_persist_supported(const TfDraftModel* model, int n, int kv_len);
int tf_draft_forward_68m_persist(const TfDraftModel* model, const TfDraftCache* cache, const int64_t* ids, int n, int slot0,
                                 int kv_len, float* logits_out, float* probs_out, float temperature, float top_p,
                                 void* ws, int64_t ws_bytes, void* ctl, void* stream);
int tf_draft_persist_tune(int key, int value);
int tf_draft_persist_stamps(void* buf);
int tf_draft_persist_error(const void* ctl);
int tf_draft_persist_reset(void* ctl, void* host_mirror, int set_mirror);

/* -------------------------------------------------------------------------------------------
 * Retrieval-cache build (models/cache.py:146-178 == :517-556): chunk-mean scoring, per-head
 * top-k, chunk gather.
 * tf_retrieval_score : scores[h][c] = fp16( q[h] . fp16(mean_{t in chunk c} K[t][h]) ), un-scaled
 *                      (cache.py:154-157).  k rows [0, C*chunk) are read once.
 *                      mean = fp16(fp32(sum * fp32(1 / chunk))), the sum in fp32 in row order
 *                      (ROUNDING OF fp16(a * b), above).
 * tf_retrieval_topk  : idx[h][0] = 0, idx[h][1..sets-1] = the sets-1 best chunks of [1,C),
 *                      descending score, ascending chunk index among equal scores
 *                      (cache.py:159-162; torch.topk leaves the tie order undefined).
 *                      ORDER: fp16 BIT-PATTERN order (sign-magnitude), so -0 sorts below +0 and
 *                      +NaN first (above +inf).  "Equal scores" (ties) means equal bit patterns:
 *                      a (+0, -0) pair is NOT a tie - it differs from IEEE equality there, and is
 *                      equally admissible against the reference's unspecified tie order.
 *                      2 <= C, 1 <= sets <= C (else TF_EINVAL); C <= 32768 (else TF_ERANGE).
 * tf_retrieval_gather: dst slot j of head h <- chunk idx[h][j] (chunk rows of D), K and V
 *                      (cache.py:163-175).
 * ------------------------------------------------------------------------------------------- */
int tf_retrieval_score(const void* k, int64_t stride_t, int64_t stride_h, const void* q,
                       void* scores, int C, int chunk, int H, int D, void* stream);
int tf_retrieval_topk(const void* scores, int32_t* idx, int C, int sets, int H, void* stream);
int tf_retrieval_gather(const void* k_src, const void* v_src, int64_t src_stride_t, int64_t src_stride_h,
                        const int32_t* idx, void* k_dst, void* v_dst, int64_t dst_stride_t,
                        int64_t dst_stride_h, int sets, int chunk, int H, int D, void* stream);

/* -------------------------------------------------------------------------------------------
 * Chunk-mean index (opt-in: RetrievalCache(index=True) / TRIFORCE_RETRIEVAL_INDEX=1).  One layer of
 * the index is [H][Cmax][D] fp16, head h at index_layer + h * index_stride_h (elements, a multiple
 * of 8, >= the chunks addressed * D).
 * tf_chunk_mean              : for every head and chunk c in [c0, c1):
 *                              index[h][c][d] = fp16( (sum_r float(K[c*chunk + r][h][d])) * (1.0f / chunk) ),
 *                              the sum in fp32 in row order, the product an fp32 value first (ROUNDING OF
 *                              fp16(a * b), above) - the mean tf_retrieval_score forms.
 *                              Chunks outside [c0, c1) are not written; c1 == c0 launches nothing.
 * tf_retrieval_score_indexed : scores[h][c] = fp16( q[h] . index[h][c] ), c < C, with the dot product
 *                              formed as tf_retrieval_score forms it behind its mean: BIT-IDENTICAL to
 *                              tf_retrieval_score over the K the index was built from.
 * D is 64 or 128.  TF_EINVAL (before anything launches) for NULL pointers, c0 < 0, c1 < c0,
 * chunk < 1, C < 1, H < 1, another D, or a stride that breaks the rule above.
 * ------------------------------------------------------------------------------------------- */
int tf_chunk_mean(const void* k, int64_t stride_t, int64_t stride_h, void* index_layer, int64_t index_stride_h,
                  int c0, int c1, int chunk, int H, int D, void* stream);
int tf_retrieval_score_indexed(const void* index_layer, int64_t index_stride_h, const void* q, void* scores,
                               int C, int H, int D, void* stream);

/* -------------------------------------------------------------------------------------------
 * KV row movement.
 * tf_kv_copy_rows : dst[l][h][dst_t0+i] = src[l][h][src_t0+i], i<n, for L layers x H heads of
 *                   D elements — RetrievalCache.update_graph_cache (cache.py:180-182, :566-575).
 *                   Source and destination must not overlap.
 * tf_kv_shift_rows: in-place move of rows [src_t0, src_t0+n) to [dst_t0, dst_t0+n), dst_t0 <=
 *                   src_t0, overlap allowed — StreamingLLMEvictionCache.evict_for_spec /
 *                   evict_prefill (cache.py:252-265).
 * ------------------------------------------------------------------------------------------- */
int tf_kv_copy_rows(const void* src, int64_t src_stride_l, int64_t src_stride_t, int64_t src_stride_h,
                    void* dst, int64_t dst_stride_l, int64_t dst_stride_t, int64_t dst_stride_h,
                    int src_t0, int dst_t0, int n, int L, int H, int D, void* stream);
int tf_kv_shift_rows(void* cache, int64_t stride_l, int64_t stride_t, int64_t stride_h,
                     int src_t0, int dst_t0, int n, int L, int H, int D, void* stream);
/* The same two movements for the K AND V tensors of one cache (equal strides and row ranges) in one launch — the two
 * tail copies and the two window shifts every decode step ends with (cache.py:180-182,252-265). */
int tf_kv_copy_rows_pair(const void* src_k, const void* src_v, int64_t src_stride_l, int64_t src_stride_t,
                         int64_t src_stride_h, void* dst_k, void* dst_v, int64_t dst_stride_l, int64_t dst_stride_t,
                         int64_t dst_stride_h, int src_t0, int dst_t0, int n, int L, int H, int D, void* stream);
int tf_kv_shift_rows_pair(void* k_cache, void* v_cache, int64_t stride_l, int64_t stride_t, int64_t stride_h,
                          int src_t0, int dst_t0, int n, int L, int H, int D, void* stream);

/* tf_kv_gather_rows: rows offset+idx[j] -> offset+j (j < n) of K and V for L layers x H heads — the compaction of
 *                   the accepted tree nodes, DistributedSimpleCache.gather_kv_incremental (cache.py:333-343).
 *                   idx (device int32) must be strictly increasing (a root-to-leaf path of the tree). */
int tf_kv_gather_rows(void* k_cache, void* v_cache, int64_t stride_l, int64_t stride_t, int64_t stride_h,
                      int offset, const int32_t* idx, int n, int L, int H, int D, void* stream);

/* -------------------------------------------------------------------------------------------
 * Dense-block glue (models/modeling_llama.py:132-159,221-238; models/tensor_op.py:25-64).
 * tf_rmsnorm    : optional fused residual add: s = fp16(x + res) (written to sum_out when
 *                 non-NULL), y = w * fp16(s * rsqrt(mean(s^2)+eps))  — the cast precedes the
 *                 weight multiply exactly as modeling_llama.py:138-143; the product inside
 *                 fp16(.) is an fp32 value first (ROUNDING OF fp16(a * b), above).
 * tf_rope_append: split a fused qkv row [q | k | v] (each H*D), rotate q (and k unless
 *                 rotate_k==0) at positions[i] with fp16 tables, write q to q_out [rows][H][D]
 *                 and the k/v rows into the cache at token slot0+i (slot0 read from slot0_dev
 *                 when non-NULL).  fp16 arithmetic order = (x*cos) + (rotate_half(x)*sin).
 * tf_silu_mul   : out = fp16(silu(gate)) * up for a fused [gate | up] row of 2*I.
 * ------------------------------------------------------------------------------------------- */
int tf_rmsnorm(const void* x, const void* res, const void* w, void* y, void* sum_out,
               int rows, int hidden, float eps, void* stream);
int tf_rope_append(const void* qkv, int64_t qkv_row_stride, const void* cos, const void* sin,
                   const int64_t* positions, void* q_out, void* k_cache, void* v_cache,
                   int64_t stride_t, int64_t stride_h, int slot0, const int32_t* slot0_dev,
                   int rows, int H, int D, int rotate_k, void* stream);
int tf_silu_mul(const void* gate_up, void* out, int rows, int I, void* stream);
/* tf_embed_rows: x = embed_tokens(input_ids) (models/modeling_llama.py:342, TP_llama.py:206) for the n <= 32 rows of a
 * decode forward, written in an explicit activation layout (see tf_skinny_gemm_act): element (m, k) at
 * out[m * out_sm + (k / 8) * out_sk + k % 8].  embed [vocab][hidden] fp16, ids [n] int64 (clamped to the vocabulary). */
int tf_embed_rows(const void* embed, const int64_t* ids, void* out, int64_t out_sm, int64_t out_sk, int n, int hidden,
                  int vocab, void* stream);
/* tf_set_tokens: the token ids, positions and length scalars of one decode forward in ONE launch; the ids (known on the
 * host: the loop has just read its accept record) travel as kernel arguments.  dst[i] = host_vals[i] for i < n_vals,
 * pad for n_vals <= i < n_dst (utils/decoding.py:94,177 — the verify / pass token rows padded with a filler id);
 * pos[i] = pos0 + i for i < n_pos (position_ids, decoding.py:178); *slot = pos0, *sk = sk_val when given (the device-side
 * lengths of a captured full-cache forward).  HOST pointer: host_vals; device pointers: dst, pos, slot, sk (each optional
 * with its count 0 / NULL).  n_dst, n_vals <= 32, n_pos <= 64. */
int tf_set_tokens(int64_t* dst, int n_dst, const int64_t* host_vals, int n_vals, int64_t pad, int64_t* pos, int n_pos,
                  int64_t pos0, int32_t* slot, int32_t* sk, int32_t sk_val, void* stream);

/* -------------------------------------------------------------------------------------------
 * Skinny (decode) GEMMs — nn.Linear / F.linear with M <= 32 activation rows (models/modeling_llama.py:
 * 156-159,212-214,243,408; models/tensor_op.py:140-142,175,353-357): y = x . W^T, fp16 in, fp32 MFMA accumulate.
 * W is passed PRE-PACKED in MFMA-operand order: [N/16 panels][K/32 chunks][64 pieces][8 fp16], piece (g*16+i)
 * of a tile = W[n0+i][k0+8g .. +7]  (triforce_amd.ops.pack_weight); N % 16 == 0, K % 32 == 0.
 * tf_skinny_gemm        : y [M][ldy] fp16, or fp32 when out_f32 != 0 (the fp16 result cast to float — `logits.float()`).
 * tf_skinny_gemm_swiglu : act [M][I] = fp16(silu(fp16(x.Wg^T))) * fp16(x.Wu^T)  — gate/up GEMMs + SwiGLU fused.
 * ------------------------------------------------------------------------------------------- */
int tf_skinny_gemm(const void* w_packed, const void* x, int64_t ldx, void* y, int64_t ldy, int M, int N, int K,
                   int out_f32, void* stream);
int tf_skinny_gemm_swiglu(const void* gate_packed, const void* up_packed, const void* x, int64_t ldx, void* act,
                          int64_t ldy, int M, int I, int K, void* stream);

/* Fused forms of the same kernel — what sits between the GEMMs of a decoder layer folded into the GEMM that consumes
 * or produces it, with the reference's rounding points (each was a 4-5 us launch of its own at <= 18 rows):
 *   ln_w != NULL : RMSNorm prologue on the input rows, h = ln_w * fp16(x * rsqrt(mean(x^2) + eps))
 *                  (models/modeling_llama.py:138-143, tensor_op.py:52-64; tf_rmsnorm's rounding points, the product
 *                  inside fp16(.) an fp32 value first: ROUNDING OF fp16(a * b), top of this file); x is then the
 *                  residual stream.
 *   resid != NULL: y = fp16(resid + fp16(x . W^T))  (hidden_states = residual + ..., modeling_llama.py:278,284);
 *                  y may alias resid (every element is read and written by the same lane).
 *   ss_out != NULL (with a fp16 output): every panel also writes sum(y[m][n]^2) over its 16 columns to
 *                  ss_out[panel * 32 + m]; ss_in != NULL (with ln_w): the norm prologue folds those N/16 partials
 *                  (of the GEMM that produced x, so K/16 of them) instead of re-reading x — the sum of squares of the
 *                  residual stream is handed from GEMM to GEMM and x is read exactly once per GEMM.
 * tf_skinny_qkv_rope: fused q|k|v projection + RoPE + KV append (modeling_llama.py:212-238 / tensor_op.py:140-160,
 *                  the work of tf_rope_append in the GEMM epilogue).  The weight must be packed in ROTARY-PAIR row
 *                  order: within the q and k sections every 16-row panel = rows d0..d0+7 and d0+D/2..d0+D/2+7 of one
 *                  head (triforce_amd.ops.rope_row_order); v rows keep their order.  q -> q_out [M][H][D]; k (rotated
 *                  unless rotate_k == 0) and v rows -> cache slot slot0 + m (slot0 read from slot0_dev if non-NULL). */
int tf_skinny_gemm_ex(const void* w_packed, const void* x, int64_t ldx, const void* ln_w, float eps,
                      const float* ss_in, const void* resid, int64_t ldr, float* ss_out, void* y, int64_t ldy,
                      int M, int N, int K, int out_f32, void* stream);
int tf_skinny_gemm_swiglu_ex(const void* gate_packed, const void* up_packed, const void* x, int64_t ldx,
                             const void* ln_w, float eps, const float* ss_in, void* act, int64_t ldy,
                             int M, int I, int K, void* stream);
int tf_skinny_qkv_rope(const void* wqkv_packed, const void* x, int64_t ldx, const void* ln_w, float eps,
                       const float* ss_in, const void* cos, const void* sin, const int64_t* positions, void* q_out,
                       void* k_cache, void* v_cache, int64_t stride_t, int64_t stride_h, int slot0,
                       const int32_t* slot0_dev, int M, int H, int D, int K, int rotate_k, void* stream);

/* The same three kernels with an explicit ACTIVATION LAYOUT per operand (round 4).  Element (m, k) of an activation
 * block lives at base[m * s_m + (k / 8) * s_k + (k % 8)]  (element strides, multiples of 8):
 *   row-major [M][ld] (the reference's tensors)            : s_m = ld, s_k = 8        — what the entry points above pass;
 *   k-octet-major, R >= M rows (triforce_amd.ops.ActBlock) : s_m = 8,  s_k = 8 * R    — the 16-byte pieces of one
 *     k-octet of all rows are contiguous, so the B operand of a 16-row MFMA tile is 4 runs of 256 B instead of 16 row
 *     fragments of 64 B.  The decode layer keeps its residual stream, attention output and SwiGLU output in this form
 *     when a block has more than 16 rows (the gamma = 16 verifies of offloading_TP.py: tensor_op.py:276-328,346-360).
 * The fp32 logits of out_f32 != 0 stay row-major (ys_m = row stride, ys_k ignored); q_out of the q|k|v form stays
 * [M][H][D].  tf_sg_tune: A/B knobs of the launch rule (csrc/sg_rule.h; key 0: rows from which a wave multiplies TWO
 * weight panels against one B operand, 33 = never; key 2: smallest halved grid, panels / 2, that takes that form; keys
 * 3-5: see tf_sg_workspace and sg_rule.h); returns the previous value, -1 for an unknown key.  Keys 1 (8 waves for the
 * two-panel form), 6 (twice the weights in flight) and 7 (batch of the narrow-panel form) are unknown keys now: those
 * variants are not buildable any more; code in the history of csrc/gemv.hip at the parent of the commit that retired
 * them; measurements in profiles/r04_draft_lm_head_launch_forms.jsonl, r04_gemm_layout_ab.jsonl and
 * r04_gemm_deep_prefetch_ab.jsonl. */
int tf_skinny_gemm_act(const void* w_packed, const void* x, int64_t xs_m, int64_t xs_k, const void* ln_w, float eps,
                       const float* ss_in, const void* resid, int64_t rs_m, int64_t rs_k, float* ss_out, void* y,
                       int64_t ys_m, int64_t ys_k, int M, int N, int K, int out_f32, void* stream);
int tf_skinny_gemm_swiglu_act(const void* gate_packed, const void* up_packed, const void* x, int64_t xs_m,
                              int64_t xs_k, const void* ln_w, float eps, const float* ss_in, void* act, int64_t ys_m,
                              int64_t ys_k, int M, int I, int K, void* stream);
int tf_skinny_qkv_rope_act(const void* wqkv_packed, const void* x, int64_t xs_m, int64_t xs_k, const void* ln_w,
                           float eps, const float* ss_in, const void* cos, const void* sin, const int64_t* positions,
                           void* q_out, void* k_cache, void* v_cache, int64_t stride_t, int64_t stride_h, int slot0,
                           const int32_t* slot0_dev, int M, int H, int D, int K, int rotate_k, void* stream);
int tf_sg_tune(int key, int value);
/* NARROW-PANEL forms of the two norm GEMMs (round 5; csrc/gemv.hip skinny_gemm_n8_kernel) for the FEW-PANEL shards of a
 * tensor-parallel rank (q|k|v: 3 * H/W * D rows, gate|up: I/W rows — 86-120 16-row panels at 8 ranks, on 256 CUs;
 * models/tensor_op.py:140-142,353-357 on the shards of models/TP_layers.py:126-147): a workgroup owns 8 output rows, two
 * 32-wide k-chunks stacked on the MFMA's 16 A rows and the matching x chunks on its 16 B columns, the two diagonal 8 x 8
 * blocks summed — twice the workgroups, half the bytes each, no cross-workgroup hand-off.  Weights packed by
 * triforce_amd.ops.pack_weight_n8 ([N/8][K/64][4][2][8][8]; q|k|v in triforce_amd.ops.rope_row_order_n8: every 8-row
 * panel of the q and k sections = rows d0..d0+3 and d0+D/2..d0+D/2+3 of one head).  Same operands, layouts and rounding
 * points as tf_skinny_gemm_swiglu_act / tf_skinny_qkv_rope_act; requires ln_w (norm prologue), M <= 24, K % 64 == 0,
 * K >= 1024 — otherwise -EINVAL and the caller keeps the 16-row form.  Results agree with the 16-row form to fp32
 * summation order (the K sum is taken even | odd chunk first), not bit for bit. */
int tf_skinny_gemm_swiglu_n8(const void* gate_n8, const void* up_n8, const void* x, int64_t xs_m, int64_t xs_k,
                             const void* ln_w, float eps, const float* ss_in, void* act, int64_t ys_m, int64_t ys_k,
                             int M, int I, int K, void* stream);
int tf_skinny_qkv_rope_n8(const void* wqkv_n8, const void* x, int64_t xs_m, int64_t xs_k, const void* ln_w, float eps,
                          const float* ss_in, const void* cos, const void* sin, const int64_t* positions, void* q_out,
                          void* k_cache, void* v_cache, int64_t stride_t, int64_t stride_h, int slot0,
                          const int32_t* slot0_dev, int M, int H, int D, int K, int rotate_k, void* stream);
/* FP8-WEIGHT forms of the three fused skinny GEMMs (csrc/gemv_fp8.hip) — the retrieval-cache ("spec") forward of the
 * target model with TRIFORCE_RETRIEVAL_WEIGHTS=fp8.  That forward only drafts: the target verify keeps
 * the fp16 weights and the accept rule keeps the output exact for the distribution the draft tokens were sampled from.
 * Numerics contract:
 *   quantization (host, triforce_amd.ops.quantize_fp8_rows, once per weight): per output row s[n] = amax_k |W[n][k]| / 448
 *     in fp32 (an all-zero row: s = 1); code = e4m3fn (OCP, not fnuz) of W / s, clamped to +-448 BEFORE the cast,
 *     rounded to nearest even.  Rows in the order the kernel reads them: q|k|v in ops.rope_row_order, gate and up apart;
 *   weight-only: activations stay fp16; the codes are decoded to fp16 exactly (scale 1.0) and multiplied on the 16-bit
 *     kernel's f16 MFMA with fp32 accumulation (no fp8 x fp8 / MX-scaled MFMA: those would quantize the activations);
 *   the row scale is applied ONCE, in fp32, on the accumulator, where the 16-bit kernel rounds: fp16(s[n] * acc) instead
 *     of fp16(acc), the scaled accumulator an fp32 value first (ROUNDING OF fp16(a * b), top of this file); gate|up: s_gate
 *     and s_up before their separate fp16 roundings.  Every other rounding point — norm
 *     prologue, residual add, SwiGLU, RoPE + append, the fp32 cast of the logits, ss_in / ss_out — is the 16-bit form's.
 * Codes packed by triforce_amd.ops.pack_weight_fp8: [N/16][K/64][4 (g)][16 (i)][16 B], the 16 bytes of piece (g, i) =
 * W[n0+i][k0+8g .. +7] then W[n0+i][k0+32+8g .. +7]: one 16x64 tile is one contiguous KiB.  `scale` / `gate_scale` /
 * `up_scale`: [N] fp32 in the same row order.  Operands, activation layouts and fused epilogues as tf_skinny_gemm_act /
 * tf_skinny_gemm_swiglu_act / tf_skinny_qkv_rope_act.  NULL codes or scales, K % 64 != 0, N % 16 != 0, M > 32 -> -EINVAL
 * before anything is launched. */
int tf_skinny_gemm_fp8_act(const void* w_fp8, const float* scale, const void* x, int64_t xs_m, int64_t xs_k,
                           const void* ln_w, float eps, const float* ss_in, const void* resid, int64_t rs_m, int64_t rs_k,
                           float* ss_out, void* y, int64_t ys_m, int64_t ys_k, int M, int N, int K, int out_f32,
                           void* stream);
int tf_skinny_gemm_swiglu_fp8_act(const void* gate_fp8, const float* gate_scale, const void* up_fp8,
                                  const float* up_scale, const void* x, int64_t xs_m, int64_t xs_k, const void* ln_w,
                                  float eps, const float* ss_in, void* act, int64_t ys_m, int64_t ys_k, int M, int I, int K,
                                  void* stream);
int tf_skinny_qkv_rope_fp8_act(const void* wqkv_fp8, const float* scale, const void* x, int64_t xs_m, int64_t xs_k,
                               const void* ln_w, float eps, const float* ss_in, const void* cos, const void* sin,
                               const int64_t* positions, void* q_out, void* k_cache, void* v_cache, int64_t stride_t,
                               int64_t stride_h, int slot0, const int32_t* slot0_dev, int M, int H, int D, int K,
                               int rotate_k, void* stream);
/* FP8 KV CACHE (csrc/kv_fp8.hip, csrc/attn.hip) — the target's full KV cache stored as OCP e4m3fn codes with
 * TRIFORCE_KV_CACHE=fp8.  TriForce stays lossless with respect to the target whose attention reads the
 * dequantized K / V, not with respect to the fp16 model.
 * Numerics contract — one exponent per (layer, head, token) row of D = 128 values, separately for K and V (K after RoPE):
 *   exponent: a = max |x| of the row (fp16 -> fp32); e = the smallest integer with 448 * 2^e >= a, clamped to [-15, 7]
 *     (an all-zero row: e = -15); stored as one uint8 per row, b = e + 127, in an [L][H][T] array for K and one for V;
 *   code = e4m3fn(clamp(x * 2^-e, -448, 448)), rounded to nearest even (x * 2^-e is exact in fp32; the clamp comes before
 *     the cast); rows with a > 57 344 saturate; NaN / Inf inputs are undefined;
 *   deq = fp16(code) * 2^e, EXACT in fp16: the smallest code step 2^-9 times 2^-15 is fp16's 2^-24, 448 * 2^7 = 57 344.
 *   Every attention read of the full cache sees deq, including the rows appended by the same forward (they are
 *   quantized before the attention that reads them).
 * Codes: [H][T][D] bytes per layer (strides in bytes); exponents: [H][exp_stride_h] bytes per layer, one per key.
 *
 * tf_kv_quant_rows: n fp16 rows of K and of V, row (h, i) at k_in / v_in + h * in_stride_h + i * in_stride_t (halves),
 *   quantized into the codes / exponents at token slot0 + i — or *slot0_dev + i when slot0_dev != NULL (the captured
 *   forward).  k_deq / v_deq (both or neither; same strides as the input, may alias it): deq is written there too.  No
 *   bounds check of the slot against the cache: the caller sizes it.  Bit-identical to the host restatement
 *   triforce_amd.ops.kv_quantize_ref.  NULL pointers, D != 128, bad strides -> -EINVAL (checked before n == 0, a no-op).
 * tf_attn_decode_fp8_act: tf_attn_decode_act over the codes (D = 128, sq <= 32).  The output is bit-identical to
 *   tf_attn_decode_act on deq(K), deq(V) with the same nsplit (same tiles, same order, same merge).  stride_t / stride_h of
 *   the codes: multiples of 16 bytes; exp_stride_h >= sk.
 * tf_kv_dequant_rows_pair: tf_kv_copy_rows_pair from codes + exponents ((L,H,T,D) byte views, exponents (L,H,T) with token
 *   stride 1) to fp16 (L,H,T,D) views: dst[l,h,dst_t0+i] = deq(src[l,h,src_t0+i]).  D = 128. */
int tf_kv_quant_rows(const void* k_in, const void* v_in, int64_t in_stride_t, int64_t in_stride_h, void* k_codes,
                     void* v_codes, void* k_exp, void* v_exp, int64_t code_stride_t, int64_t code_stride_h,
                     int64_t exp_stride_h, int slot0, const int32_t* slot0_dev, int n, int H, int D, void* k_deq,
                     void* v_deq, void* stream);
int tf_attn_decode_fp8_act(const void* q, const void* k_codes, const void* v_codes, const void* k_exp, const void* v_exp,
                           void* out, int64_t out_sm, int64_t out_sk, int64_t stride_t, int64_t stride_h,
                           int64_t exp_stride_h, int sq, int sk, const int32_t* sk_dev, int H, int D, float scale,
                           int nsplit, float* ws, int64_t ws_floats, uint32_t* tickets, void* stream);
int tf_kv_dequant_rows_pair(const void* src_k, const void* src_v, int64_t src_stride_l, int64_t src_stride_t,
                            int64_t src_stride_h, const void* exp_k, const void* exp_v, int64_t exp_stride_l,
                            int64_t exp_stride_h, void* dst_k, void* dst_v, int64_t dst_stride_l, int64_t dst_stride_t,
                            int64_t dst_stride_h, int src_t0, int dst_t0, int n, int L, int H, int D, void* stream);
/* FP8 RETRIEVAL CACHE (csrc/kv_fp8.hip, csrc/attn.hip) — the retrieval cache's rows [0, max_budget) stored in the row format
 * above with TRIFORCE_RETRIEVAL_KV=fp8: codes [L][H][max_budget][128] and exponent bytes
 * [L][H][max_budget], separately for K and V; no new numerics.  The gamma + 1 rows a retrieval-cache (spec) forward appends
 * are scratch — every such forward rewrites them, the durable copy arrives through the tail refresh from the full cache —
 * and stay fp16 in a small [L][H][gamma + 1][128] array.  The middle tier only drafts, so the decoding stays lossless with
 * respect to the target for any such storage.
 * Both row movers take either source: fp16 rows (src exponent pointers NULL; strides in halves) are quantized by the contract
 * above, bit-identical to triforce_amd.ops.kv_quantize_ref; codes + exponents (strides in bytes, multiples of 16; exponents
 * with token stride 1) are copied byte for byte — the middle tier then reads exactly the deq the target reads.  K and V in
 * one launch.  D = 128.  NULL pointers, one source exponent pointer without the other, bad strides -> -EINVAL (checked
 * before n == 0, a no-op).  No bounds check of rows or chunk ids against the arrays: the caller sizes them.
 *
 * tf_retrieval_gather_fp8: tf_retrieval_gather of one layer into codes: destination row s * chunk + r of head h = source row
 *   idx[h][s] * chunk + r, s < sets, r < chunk.  exp_stride_h >= sets * chunk.
 * tf_kv_quant_rows_pair: tf_kv_copy_rows_pair into codes over L layers: dst[l,h,dst_t0+i] = src[l,h,src_t0+i], i < n (the
 *   refresh of the generated tail).
 * tf_attn_decode_fp8_tail_act: tf_attn_decode_fp8_act whose keys [0, sk_codes) are codes + exponents and whose keys
 *   [sk_codes, sk_codes + n_tail) are fp16 rows, row (h, i) at k_tail / v_tail + h * tail_stride_h + i * tail_stride_t
 *   (halves, multiples of 8).  The source is picked per key row while the wave-private staging tile is filled, so a 16-key
 *   tile may straddle the boundary; fragments, tile order, split rule and both merges are tf_attn_decode_act's: the output is
 *   bit-identical to tf_attn_decode_act on [deq(codes) | tail rows] with the same nsplit, in either output layout.
 *   D = 128, sq <= 32, 1 <= n_tail <= 32, sk_codes >= 1, exp_stride_h >= sk_codes; sk_dev must be NULL (the boundary is a
 *   host value); anything else -> -EINVAL before any launch. */
int tf_retrieval_gather_fp8(const void* k_src, const void* v_src, int64_t src_stride_t, int64_t src_stride_h,
                            const void* k_src_exp, const void* v_src_exp, int64_t src_exp_stride_h, const int32_t* idx,
                            void* k_codes, void* v_codes, void* k_exp, void* v_exp, int64_t code_stride_t,
                            int64_t code_stride_h, int64_t exp_stride_h, int sets, int chunk, int H, int D, void* stream);
int tf_kv_quant_rows_pair(const void* src_k, const void* src_v, int64_t src_stride_l, int64_t src_stride_t,
                          int64_t src_stride_h, const void* src_exp_k, const void* src_exp_v, int64_t src_exp_stride_l,
                          int64_t src_exp_stride_h, void* k_codes, void* v_codes, int64_t code_stride_l,
                          int64_t code_stride_t, int64_t code_stride_h, void* k_exp, void* v_exp, int64_t exp_stride_l,
                          int64_t exp_stride_h, int src_t0, int dst_t0, int n, int L, int H, int D, void* stream);
int tf_attn_decode_fp8_tail_act(const void* q, const void* k_codes, const void* v_codes, const void* k_exp, const void* v_exp,
                                const void* k_tail, const void* v_tail, void* out, int64_t out_sm, int64_t out_sk,
                                int64_t stride_t, int64_t stride_h, int64_t exp_stride_h, int64_t tail_stride_t,
                                int64_t tail_stride_h, int sq, int sk_codes, int n_tail, const int32_t* sk_dev, int H, int D,
                                float scale, int nsplit, float* ws, int64_t ws_floats, uint32_t* tickets, void* stream);
/* Split-K workspace of the CURRENT device (csrc/gemv.hip, SgKsplit): GEMMs with few output panels — the q|k|v and
 * gate|up shards of a tensor-parallel rank — split K across up to 4 workgroups per panel; their partial sums meet in
 * `ws` (zero-filled device memory, first 16 KiB = per-panel tickets, left zero by every launch; 8 MiB covers every shape
 * the rule splits), summed in split order by the last workgroup to arrive.  Without a registered workspace no GEMM is
 * split.  The workspace is cut into 4 equal slots, one per LAUNCH STREAM (first come, first served): split GEMMs on different
 * streams of one device may run concurrently; a fifth stream's GEMMs run unsplit.  ws = NULL removes it.  (tf_sg_tune key
 * 3: panel-group count below which the split applies, 0 = never.) */
int tf_sg_workspace(void* ws, int64_t bytes);

/* -------------------------------------------------------------------------------------------
 * Sampling / accept-rollback (utils/sampling.py:63-75, utils/decoding.py:97-134,190-220).
 * tf_sample_inverse_cdf: token = first index whose inclusive cumulative sum of probs exceeds
 *                        u * sum(probs)  (stand-in for torch.multinomial with an explicit uniform).
 *                        Only an index with non-zero mass is ever returned.  When no cumulative sum
 *                        exceeds u * sum(probs) (u = 1.0 reaches the total exactly, or the product
 *                        rounds past it) the token is the LAST index with non-zero mass, not V - 1.
 *                        A row with no mass at all (every entry <= 0) gives token 0.  The same two
 *                        rules hold for every draw below: the residual, the bonus and the follow-up
 *                        sample, and the final draw of tf_tree_accept.
 * tf_accept_chain      : sequential speculative accept test of g2 drafted tokens against the
 *                        target distribution rows p[0..g2] and the drafting rows q[0..g2-1]:
 *                        flag_i = u_i < min(1, p_i[x_i]/q_i[x_i])  (<= when inclusive), count =
 *                        accepted prefix (wave ballot + ffs), stop at an accepted eos; then the
 *                        correction token: residual max_fn(p_count - q_count) on rejection, bonus
 *                        p_g2 when everything passed.  The sample uses uniforms[examined].
 *                        out[0]=count, out[1]=next token, out[2]=reason (0 rejected, 1 all
 *                        accepted, 2 eos accepted), out[3]=number of uniforms consumed.
 * tf_middle_accept     : one inner TriForce step (decoding.py:190-220): test drafted token d
 *                        (= tokens[n+1]) with p[n], q_d; sample the follow-up token from p[n+acc].
 *                        out[0]=accepted(0/1), out[1]=follow-up token.  Also writes the follow-up
 *                        token into tokens[n+1+acc] when that index is <= gamma.
 * ------------------------------------------------------------------------------------------- */
/* tf_topp_probs: probs = softmax(top_p_filter(logits / temperature)) for `rows` rows of V <= 32768 fp32 logits —
 * utils/sampling.py:43-60 (norm_logits with top_k = -1) without the vocabulary sort: threshold search on the
 * fp32 bit pattern + index-ordered tie scan (== a stable descending sort; ties -> lowest token id). */
int tf_topp_probs(const float* logits, float* probs, int rows, int V, float temperature, float top_p, void* stream);
/* tf_topk_topp_probs: tf_topp_probs behind the reference's top-k filter (utils/sampling.py:16-19) — the target tier's sampling
 * with top_k > 0 (first token, target verify, autoregressive baseline), one launch, no vocabulary sort.  Per row:
 *   x_i = l_i / temperature (IEEE fp32 division, as in tf_topp_probs);
 *   kth = the min(top_k, V)-th largest x, counted with multiplicity;
 *   survivors S = { i : x_i >= kth } — EVERY entry tied with the k-th value survives (the reference masks `logits < kth`, it
 *   does not keep "exactly k"); -0.0 and +0.0 compare equal; a -inf logit is legal (mass 0; it survives only if kth is -inf);
 *   NaN is outside the contract.
 * Entries outside S get probability 0 and contribute to no sum.  Over S the result is exactly what tf_topp_probs defines:
 * e_i = expf(x_i - max), masses as 2^-40 fixed-point integers, tau = floor(top_p * Z) with Z summed over S only, the boundary
 * by radix select on mass, ties at the boundary kept in index order, outputs e_i / Zk.  top_k >= V filters nothing: the output
 * is then BIT-IDENTICAL to tf_topp_probs.  kth comes from a radix select on integer COUNT histograms, so nothing depends on the
 * order in which atomics land.  One workgroup of 1 024 threads per row.
 * TF_EINVAL: NULL pointer, rows < 1, V < 1, !(temperature > 0), !(top_p > 0), top_k < 1.  TF_ERANGE: V > 32768. */
int tf_topk_topp_probs(const float* logits, float* probs, int rows, int V, float temperature, int top_k, float top_p,
                       void* stream);
/* tf_topp_probs_large / tf_topk_topp_probs_large (csrc/topp_large.hip): the two normalisers above for
 * vocabularies up to 262 144 (Z < 2^58 still fits the 64-bit sums), 1 <= rows <= 32, any V (also V % 4 != 0), any 4-byte-aligned
 * base, contiguous rows.  The numerics are EXACTLY those stated for tf_topp_probs and tf_topk_topp_probs — the same helpers
 * decide every bit — so for V <= 32768 the output is BIT-IDENTICAL to the kernel of the same name without _large.  One workgroup
 * of 1 024 threads per row; the row (x, then e) and the candidates of the select stream through `ws` instead of living in LDS.
 *   ws   >= TF_TOPP_LARGE_WS_BYTES(rows, V) bytes of device scratch, 16-byte aligned: per row the x / e values and the candidate
 *        list, each padded to whole slabs of 4 096 entries (a macro, not a call: the size is pure arithmetic on the shape).  It
 *        carries no state between launches (nothing to zero, graph replays may run back to back); launches that share one ws
 *        must be ordered against each other (one stream, or a graph's edges).
 * No host synchronisation and no allocation: capturable in a hipGraph.  All gates come before anything launches:
 * TF_EINVAL: NULL pointer (ws included) or misaligned ws, rows < 1, rows > 32, V < 1, !(temperature > 0), !(top_p > 0),
 * top_k < 1.  TF_ERANGE: V > 262144.  TF_ENOSPC: ws_bytes too small.  top_k >= V is tf_topp_probs_large bit for bit. */
#define TF_TOPP_LARGE_MAX_VOCAB 262144
#define TF_TOPP_LARGE_WS_BYTES(rows, V) ((int64_t)(rows) * ((((int64_t)(V) + 4095) >> 12) * 4096 * 2) * 4)
int tf_topp_probs_large(const float* logits, float* probs, int rows, int V, float temperature, float top_p, void* ws,
                        int64_t ws_bytes, void* stream);
int tf_topk_topp_probs_large(const float* logits, float* probs, int rows, int V, float temperature, int top_k, float top_p,
                             void* ws, int64_t ws_bytes, void* stream);
/* tf_minp_probs / tf_minp_probs_large: the normalisers above with a MIN-P filter behind the top-p select
 * (HF order: temperature -> top-k -> top-p -> min-p) — the target tier's sampling with min_p > 0.  top_k <= 0 or top_k >= V
 * means no top-k filter; one entry serves both forms.  With x, the top-k survivors S, e_i = expf(x_i - max), the masses, Z, tau
 * and the kept set K exactly as tf_topp_probs / tf_topk_topp_probs define them,
 *   K' = { i in K : e_i >= min_p }   (compared in fp32; for non-negative floats a comparison of bit patterns),
 * outputs e_i / Zk' on K' and 0 elsewhere, Zk' the exact integer sum of the 2^-40 fixed-point masses over K', converted as Zk
 * is.  The row maximum has e = expf(0) = 1.0f exactly, so no normaliser enters the rule: a softmax over any masked set has the
 * ratios p_i / p_max = e_i, hence the rule is HF's p_i >= min_p * p_max up to its float rounding.  Consequences, with ustar the
 * boundary pattern of the top-p select and umin = bits(min_p):
 *   umin <= ustar: min-p removes nothing and the output is BIT-IDENTICAL to the entry without min-p;
 *   otherwise K' = { bits(e_i) >= umin }: the boundary ties are gone, Zk' takes one more exact reduction over the row;
 *   min_p = 1.0 keeps exactly the entries equal to the row maximum: a unique maximum gives a one-hot row of exactly 1.0, equal
 *   maxima share the mass.  A -inf logit is legal (mass 0); NaN is outside the contract.
 * tf_minp_probs: V <= 32768, any rows.  tf_minp_probs_large: V <= 262144, rows <= 32, ws as for tf_topp_probs_large
 * (TF_TOPP_LARGE_WS_BYTES); for V <= 32768 bit-identical to tf_minp_probs.  One workgroup of 1 024 threads per row, no state
 * between launches, capturable.  All gates come before anything launches:
 * TF_EINVAL: NULL pointer, rows < 1, V < 1, !(temperature > 0), !(top_p > 0), !(min_p > 0), min_p > 1 (_large: rows > 32, a NULL
 * or misaligned ws).  TF_ERANGE: V above the entry's limit.  TF_ENOSPC: ws_bytes too small. */
int tf_minp_probs(const float* logits, float* probs, int rows, int V, float temperature, int top_k, float top_p, float min_p,
                  void* stream);
int tf_minp_probs_large(const float* logits, float* probs, int rows, int V, float temperature, int top_k, float top_p,
                        float min_p, void* ws, int64_t ws_bytes, void* stream);
int tf_sample_inverse_cdf(const float* probs, const float* u, int64_t* token_out, int V, void* stream);
int tf_accept_chain(const float* p, const float* q, const int64_t* tokens, const float* uniforms,
                    int g2, int V, int inclusive, int64_t eos_token_id, int64_t* out, void* stream);
int tf_middle_accept(const float* p, const float* q_d, int64_t* tokens, const float* uniforms,
                     int n, int gamma, int V, int64_t* out, void* stream);
/* tf_mid_record_tokens: tokens[n + 1] (, tokens[n + 2]) as a tf_middle_accept record (accepted, follow-up, drafted) implies —
 * the tensor-parallel loop applies RANK 0's broadcast record (utils/decoding.py:452-470) with it in one launch. */
int tf_mid_record_tokens(const int64_t* rec, int64_t* tokens, int tokens_len, int n, void* stream);
/* tf_topp_probs_multi (csrc/topp_multi.hip; round 6): tf_topp_probs with every row spread over 16 (8 from 17 rows up) workgroups of
 * ONE launch — every workgroup takes the row maximum from the whole row (tune key 3 = 0: the slices exchange their maxima through
 * an in-launch edge instead), the slices of a row meet through an in-launch edge (mass sums + compacted candidates), then every
 * workgroup of the row runs the exact-integer select over the row's candidates and writes its own entries.  Probabilities are
 * BIT-IDENTICAL to tf_topp_probs (utils/sampling.py:5-27,43-60).  rows <= 32, V % 4 == 0, 64 <= V <= 32768, rows x slices <= the
 * device's CU count (TF_ERANGE otherwise: the caller keeps tf_topp_probs).
 *   panel_max  NULL, or [V / 16][32] fp32: per-16-column-panel row maxima of the logits as the lm_head GEMM's epilogue leaves them
 *              (tf_skinny_gemm_act with out_f32 = 1 and ss_out != NULL): the first edge is skipped
 *   ctl        tf_topp_multi_ctl_bytes() bytes, 64-byte aligned, ZERO-filled once; launches on one ctl must not overlap
 *   ws         >= tf_topp_multi_ws_bytes(rows, V) bytes of device scratch, 256-byte aligned
 * Bounded waits (tf_topp_multi_tune key 0 = ms, default 2000; key 1 = fault injection for tests; key 2 = entries of the LDS
 * candidate list; key 3 = where the row maximum comes from): a time-out sets the sticky
 * error word (tf_topp_multi_error) and NaN-fills the rows until tf_topp_multi_reset. */
int64_t tf_topp_multi_ctl_bytes(void);
int64_t tf_topp_multi_ws_bytes(int rows, int V);
int tf_topp_probs_multi(const float* logits, const float* panel_max, float* probs, int rows, int V, float temperature,
                        float top_p, void* ctl, void* ws, int64_t ws_bytes, void* stream);
int tf_topp_multi_tune(int key, int value);
int tf_topp_multi_error(const void* ctl);
int tf_topp_multi_reset(void* ctl);

/* The same three kernels with their uniforms behind a DEVICE CURSOR (round 5): u_k = ubuf[*cursor + k] — the form that
 * can sit INSIDE a captured hipGraph (frozen arguments, fresh numbers at every replay), which is how the inner loop of
 * utils/decoding.py:163-223 becomes ONE graph launch per iteration (draft forward, draw, retrieval verify, accept test).
 *   tf_sample_inverse_cdf_cur: u = ubuf[*cursor + off]; the cursor is left alone.
 *   tf_middle_accept_cur     : accept test with ubuf[*cursor + 1], follow-up sample with ubuf[*cursor + 2]; *cursor += 3;
 *                              out[3] = the cursor value the decision started from (the host checks its mirror).
 *   tf_accept_chain_cur      : the chain over ubuf[*cursor ...]; *cursor += out[3].
 * In ALL forms (cursor or not) what the kernel leaves for the next chain of launches on the device — the token id in
 * `tokens`, the cursor — is stored write-through (agent scope) and drained BEFORE the record `out` is stored.  CONTRACT: a
 * host that polls `out` in pinned memory may enqueue the next chain the moment it sees the record ONLY ON THE SAME STREAM
 * (stream order then also orders the chain behind this kernel's completion).  A chain on another stream is ordered by the
 * record alone, which the runtime knows nothing about: its first kernel would need an explicit agent-scope acquire of what it
 * reads, and none of the entry points does that (the two-stream loop of round 5 was removed for this reason). */
int tf_sample_inverse_cdf_cur(const float* probs, const float* ubuf, const int64_t* cursor, int off, int64_t* token_out,
                              int V, void* stream);
int tf_middle_accept_cur(const float* p, const float* q_d, int64_t* tokens, int tokens_len, const float* ubuf,
                         int64_t* cursor, int n, int gamma, int V, int64_t* out, void* stream);
int tf_accept_chain_cur(const float* p, const float* q, const int64_t* tokens, const float* ubuf, int64_t* cursor, int g2,
                        int V, int inclusive, int64_t eos_token_id, int64_t* out, void* stream);
/* tf_middle_accept_cur: a `tokens` buffer of >= gamma + 2 entries (the engine's shared token buffer) also receives the
 *   follow-up token of the LAST position (index gamma + 1), so that after the inner loop it holds all of [next, t_1 .. t_g2].
 * tf_accept_chain_step: tf_accept_chain_cur over tok_buf[1 ..] that also leaves on the device what follows its record
 *   (utils/decoding.py:124,137): tok_buf[0 .. g2 + 1] = the PASS TOKENS of the catch-up draft forward ([next, accepted ...,
 *   resampled | bonus token, pad ...]; pad in its place after an accepted eos), and for nsets <= 2 captured target-verify lengths
 *   the positions (n_pos entries from S'), append slot (S') and key count (S' + qlen) of the NEXT verify, S' = *s_src + count + 1
 *   = the cache length after the roll-back (s_src: the append slot of the verify just run).  Neither the catch-up draft nor the
 *   next target verify then needs a set-up launch behind a record read.  tok_len >= g2 + 2; g2 <= 62. */
/* tf_middle_accept2_cur: up to `depth` (1 or 2) successive inner positions n, n + 2 decided from ONE
 *   retrieval verify.  The caller ran the draft ahead: tokens[n + 1] = d ~ q1 with ubuf[c]; tokens[n + 2] = a guess of the follow-up
 *   token (drawn from the draft's next row with ubuf[c + 2], the uniform the follow-up itself uses); tokens[n + 3] ~ q3 with
 *   ubuf[c + 3] (c = *cursor).  Stage 1 is tf_middle_accept_cur's arithmetic (one shared device function).  If it accepts AND its
 *   follow-up equals tokens[n + 2], stage 2 decides position n + 2 from rows n + 2, n + 3 of p with ubuf[c + 4], ubuf[c + 5],
 *   writes tokens[n + 3 + acc2] and sets *cursor = c + 6; otherwise tokens[n + 1 + acc1] and *cursor = c + 3, exactly as
 *   tf_middle_accept_cur.  out[8] (depth 2; 5 for depth 1) = (acc1, b1, d1, c, stage2_ran, acc2, b2, d2), zeros for a stage that
 *   did not run, every entry written.  n + 2 (depth - 1) + 1 <= gamma; same store order and stream contract as above. */
int tf_middle_accept2_cur(const float* p, const float* q1, const float* q3, int64_t* tokens, int tokens_len, const float* ubuf,
                          int64_t* cursor, int n, int gamma, int V, int depth, int64_t* out, void* stream);
/* tf_middle_accept_n_cur: the N-stage form of tf_middle_accept2_cur, depth 1 .. 4 successive inner positions
 *   n, n + 2, n + 4, .. decided from ONE retrieval verify by the same kernel.  One draft row per stage: tokens[n + 2s + 1] ~ q1,
 *   q3, q5, q7 with ubuf[c + 3s]; tokens[n + 2s] (s >= 1) a guess of stage s - 1's follow-up token drawn with ubuf[c + 3(s-1) + 2].
 *   Stage s runs iff every earlier stage accepted and its follow-up equals the guess; it uses ubuf[c + 3s + 1], ubuf[c + 3s + 2].
 *   Only the last stage that ran writes its follow-up token; *cursor = c + 3 x stages run.  out[5 + 3 (depth - 1)] = (acc, b, d, c,
 *   further stages run, then (acc, b, d) per further stage, zeros for a stage that did not run), every entry written; out_len is
 *   the room behind `out`.  n + 2 (depth - 1) + 1 <= gamma; a non-null row for every stage up to depth; rows beyond may be NULL. */
int tf_middle_accept_n_cur(const float* p, const float* q1, const float* q3, int64_t* tokens, int tokens_len, const float* ubuf,
                           int64_t* cursor, int n, int gamma, int V, int depth, int64_t* out, void* stream, const float* q5,
                           const float* q7, int out_len);
int tf_accept_chain_step(const float* p, const float* q, int64_t* tok_buf, int tok_len, const float* ubuf, int64_t* cursor,
                         int g2, int V, int inclusive, int64_t eos_token_id, int64_t pad, const int32_t* s_src, int nsets,
                         int64_t* pos_a, int n_pos_a, int32_t* slot_a, int32_t* sk_a, int qlen_a, int64_t* pos_b, int n_pos_b,
                         int32_t* slot_b, int32_t* sk_b, int qlen_b, int64_t* out, void* stream);

/* -------------------------------------------------------------------------------------------
 * Sequoia tree verification (utils/SpecTree_TP.py:147-199: accept_step + the walk in verify()).
 *   p_rows        [N][V] fp32 target probabilities of every tree node (top-p filtered softmax)
 *   draft_logits  [N][V] fp32 draft logits of every node (q = softmax(draft_logits / temperature), with the
 *                 rejected sibling tokens removed, as :159-166)
 *   tokens        [N] int64 token of every node;  succ_off [N+1], succ: CSR of grow_map["Successors"]
 *   uniforms      fp32 stream: one per examined child, then one for the residual sample
 *   out int64 [4 + 60]: out[0] = len(accept_list) incl. the root, out[1] = next token, out[2] = terminal
 *                 (accepted token 0 / 2, or a NaN residual), out[3] = uniforms consumed, out[4+j] = accept_list[j]
 * One single-workgroup launch replaces the reference's host loop (one device sync per examined child).  V <= 32768.
 * ------------------------------------------------------------------------------------------- */
int tf_tree_accept(const float* p_rows, const float* draft_logits, const int64_t* tokens,
                   const int32_t* succ_off, const int32_t* succ, const float* uniforms, int V,
                   float temperature, int64_t* out, void* stream);

/* Sampling WITHOUT replacement for the tree growth (test/offloading_seqouia.py:29-39):
 * out[row][0..k) = the k token ids with the largest log(rand[row][i]) / softmax(logits[row] / temperature)[i], in
 * descending order (= `(rand.log() / q).topk(k).indices`); rand is fp16, logits fp32 [rows][V]; k <= 16, V <= 32768.
 * One kernel instead of softmax + log + div + multi-block top-k (which also hangs when replayed from a hipGraph). */
int tf_sample_without_replacement(const float* logits, const void* rand_f16, int64_t* out, int rows, int V, int k,
                                  float temperature, void* stream);

/* -------------------------------------------------------------------------------------------
 * Offloading tier (models/cache.py:345-351 copy_back_from_buffer, :372-376 copy_kv, :573-575):
 * asynchronous pinned-host <-> device copies of a head-major KV block = H rows of width_elems
 * contiguous fp16 (n tokens x D) at the given pitches (in elements).  Enqueued on `copy_stream`
 * (hipMemcpy2DAsync); the caller orders them against compute with events — no device-wide syncs.
 * *_host pointers are HOST pointers to pinned memory.
 * ------------------------------------------------------------------------------------------- */
int tf_kv_h2d_async(void* dst_dev, int64_t dst_pitch_elems, const void* src_host, int64_t src_pitch_elems,
                    int64_t width_elems, int H, void* copy_stream);
int tf_kv_d2h_async(void* dst_host, int64_t dst_pitch_elems, const void* src_dev, int64_t src_pitch_elems,
                    int64_t width_elems, int H, void* copy_stream);

/* -------------------------------------------------------------------------------------------
 * One-shot all-reduce over peer-mapped buffers (xGMI) — replaces dist.all_reduce at models/tensor_op.py:179,326,359
 * for the 57..184 KB decode messages of the tensor-parallel path (2 per layer and forward; a ring collective pays
 * 2(W-1) latency hops on each).  Every rank stages its fp16 partial in a FINE-GRAINED buffer its peers have mapped
 * (tf_ar_alloc + tf_ar_get_ipc_handle / tf_ar_open_ipc_handle), exchanges one READY flag, reads all partials and adds
 * them in rank order with fp32 accumulation (bit-identical on every rank), then exchanges one DONE flag so the staging
 * buffer can be reused when the kernel ends.  The epoch lives in the control block: capturable in a hipGraph.  All
 * spins are bounded (tf_ar_error != 0 afterwards = a peer never arrived; from then on every call fills `out` with NaN
 * and returns at once — the host polls tf_ar_error once per decode step).
 *   peer_data / peer_flags : `world` device-visible pointers (own entry included); this rank's partial must already be
 *                            in peer_data[rank], written by an earlier kernel of `stream`; n % 8 == 0 fp16 elements;
 *                            `out` is ordinary device memory, not the staging buffer.
 * ------------------------------------------------------------------------------------------- */
int tf_ar_flags_bytes(void);
int tf_ar_ipc_handle_bytes(void);
int tf_ar_alloc(int64_t bytes, void** ptr);
int tf_ar_free(void* ptr);
int tf_ar_get_ipc_handle(void* ptr, void* handle_out);
int tf_ar_open_ipc_handle(const void* handle, void** ptr_out);
int tf_ar_close_ipc_handle(void* ptr);
int tf_allreduce_oneshot(void* const* peer_data, void* const* peer_flags, int rank, int world, void* out, int64_t n,
                         void* stream);
/* out = resid + all_reduce(partials): `hidden_states = residual + all_reduce(...)` (tensor_op.py:179-181,359-360) in the
 * same launch; the residual is added in fp16 to the ROUNDED sum (the reference's two rounding points); resid may be
 * `out` itself (in-place residual stream), NULL = plain all-reduce. */
int tf_allreduce_oneshot_add(void* const* peer_data, void* const* peer_flags, int rank, int world, const void* resid,
                             void* out, int64_t n, void* stream);
/* ... plus the per-panel sums of squares of the result rows (out = [n / hidden][hidden], <= 32 rows):
 * ss_out[panel * 32 + row], the hand-off tf_skinny_gemm_ex folds as ss_in — the RMSNorm after an all-reduce
 * (tensor_op.py:52-64 after :179 / :359) then runs in the prologue of the next GEMM without re-reading the rows. */
int tf_allreduce_oneshot_add_ss(void* const* peer_data, void* const* peer_flags, int rank, int world, const void* resid,
                                void* out, int64_t n, int hidden, float* ss_out, void* stream);
/* Alternating form: every staging buffer holds 2 * half_elems values and exchange e (the control block's epoch, 1 for
 * the first exchange after tf_ar_alloc) uses the half e & 1, which removes the closing DONE handshake: a rank cannot
 * overwrite a half before every peer has signalled READY for the exchange in between (csrc/allreduce.hip header).
 * `expect_half` = the half this rank's producer wrote; if the epoch selects the other one the call fills `out` with NaN
 * and sets the sticky error 3.  resid and ss_out may be NULL (hidden is read only with ss_out).  One form per control
 * block for its lifetime, the same on every rank. */
int tf_allreduce_oneshot_alt(void* const* peer_data, void* const* peer_flags, int rank, int world, const void* resid,
                             void* out, int64_t n, int hidden, float* ss_out, int64_t half_elems, int expect_half,
                             void* stream);
/* tf_allreduce_oneshot_add_ss / _alt for a residual stream kept k-octet-major (tf_skinny_gemm_act): n = pack_rows *
 * hidden elements, piece i = (k-octet i / pack_rows, row i % pack_rows); ss_out[panel * 32 + row] as above (required).
 * half_elems == 0: the READY / reduce / DONE form; > 0: alternating halves with expect_half. */
int tf_allreduce_oneshot_act(void* const* peer_data, void* const* peer_flags, int rank, int world, const void* resid,
                             void* out, int64_t n, int hidden, int pack_rows, float* ss_out, int64_t half_elems,
                             int expect_half, void* stream);
/* GEMM + all-reduce in ONE launch (csrc/gemv.hip, SgXchg) — o_proj / down_proj of the tensor-parallel decode layer with
 * their exchange in the GEMM epilogue: out = resid + sum over ranks of fp16(x . W^T)  (models/tensor_op.py:175-181,
 * 353-360; the arithmetic of tf_skinny_gemm_act(out = staging) + tf_allreduce_oneshot_add_ss).  Every workgroup publishes
 * its 16-column panel in this rank's staging half (half = device epoch & 1), flags the same panel on every peer, waits for
 * the peers' flags of that panel, reads their panels and finishes — no grid-wide wait, no DONE phase, no host-side half.
 * peer_stage[r] / peer_ctl[r], r < world: every rank's staging buffer (2 * half_elems fp16) and control buffer
 * (tf_xchg_ctl_bytes() bytes, zero-filled once), fine-grained memory (tf_ar_alloc), own entries included, peers' mapped
 * through hipIpc (tf_ar_get_ipc_handle / tf_ar_open_ipc_handle).  The result block `out` (may alias resid) and the
 * staging halves share the activation layout (os_m, os_k); N / 16 <= 512; the block must fit a half.  ss_out: per-panel
 * sums of squares of the result rows (may be NULL).  Bounded spins: a time-out NaN-fills the panel and sets the sticky
 * error word (tf_xchg_error; tf_xchg_set_error(ctl, code, host_mirror, set_mirror) injects / clears it and registers a
 * pinned host word that mirrors it). */
int64_t tf_xchg_ctl_bytes(void);
int tf_skinny_gemm_xchg(const void* w_packed, const void* x, int64_t xs_m, int64_t xs_k, void* const* peer_stage,
                        void* const* peer_ctl, int rank, int world, int64_t half_elems, const void* resid, int64_t rs_m,
                        int64_t rs_k, void* out, int64_t os_m, int64_t os_k, float* ss_out, int M, int N, int K,
                        void* stream);
int tf_xchg_error(const void* ctl);
int tf_xchg_set_error(void* ctl, int code, void* host_mirror, int set_mirror);
/* tf_xchg_tune: key 0 = FENCED form of the exchange (1: system-scope release before the flag stores and acquire behind the
 *   flag wait, the pair the first build had, ~1.7 us each; 0, default: s_waitcnt vmcnt(0) + system-scope accesses in issue
 *   order) — selected by the engine's start-up litmus on the real group (utils/oneshot_ar.GemmExchange.litmus) when the
 *   fence-free form shows a single mismatch, or forced with TRIFORCE_XCHG_FENCE=1; key 1 = wall-clock limit of one flag wait
 *   in milliseconds (default 5000: a dead or starved peer is reported in seconds, not after 2^27 polls).  Returns the
 *   previous value (a value outside the key's range only reads), -1 for an unknown key.
 * tf_xchg_reset: control block back to its freshly allocated state (peer flags, per-panel exchange counts, error word; the
 *   host mirror stays registered).  COLLECTIVE by contract: all ranks, between two barriers, nothing in flight. */
int tf_xchg_tune(int key, int value);
int tf_xchg_reset(void* ctl);
/* Message-passing litmus around the exchange (tools/xgmi_litmus.py): tf_ar_litmus_stage advances the device counter
 * *it_dev and then writes, with PLAIN stores from an ordinary kernel (the role of the o_proj / down_proj epilogue), the
 * pattern v_rank[i] = (7 i + 13 it + 101 rank) mod 509 into `staging` (n fp16 values); after an all-reduce of those
 * partials tf_ar_litmus_check adds to *bad (uint64, device) the number of elements of `out` that differ from
 * fp16(sum over ranks of v_r[i]) for the same iteration.  Both are capturable. */
int tf_ar_litmus_stage(void* staging, int64_t n, int rank, uint32_t* it_dev, void* stream);
int tf_ar_litmus_check(const void* out, int64_t n, int world, const uint32_t* it_dev, uint64_t* bad, void* stream);
int tf_ar_error(const void* flags_local);
/* completed exchanges of this control block (device-side epoch), blocking host read: lets a caller that counts its
 * exchanges (expect_half) resynchronise after a failed launch / capture; TF_EINVAL for NULL, -(hip error) on failure */
int64_t tf_ar_epoch(const void* flags_local);
/* host_word: pinned, device-mapped host memory (4 bytes) that receives every error code the kernels set from now on (and
 * the current one at once) — the per-step health poll then reads host memory instead of copying the control block;
 * NULL removes the mirror.  The word must outlive the control block. */
int tf_ar_set_error_mirror(void* flags_local, void* host_word);
/* Fault injection for tests: sets (code > 0) or clears (0) the sticky error word of a control block from the host. */
int tf_ar_inject_error(void* flags_local, int code);

/* -------------------------------------------------------------------------------------------
 * GROUPED-QUERY ATTENTION: H query heads over Hkv = H / g KV heads, query head h reads KV head h / g —
 * the reference's repeat_kv (models/tensor_op.py:8-17) in front of flash_attn_with_kvcache (models/modeling_llama.py:240;
 * its projections at :213-215 and its caches, models/cache.py:20-61, already take num_key_value_heads).  Each entry is its
 * multi-head neighbour with two head counts; H % Hkv != 0, sizes < 1, NULL buffers and D other than 64 / 128 -> TF_EINVAL.
 * tf_attn_decode_gqa_act: tf_attn_decode_act (models/modeling_llama.py:240 for verify / decode blocks of sq <= 32 rows).
 *   The sq token rows of gs query heads of one KV head are stacked into one gs * sq <= 32 row problem of the split-KV
 *   kernel, gs = the largest divisor of g with gs * sq <= 32; a KV head has g / gs such sub-groups, each its own workgroup
 *   column (cols = Hkv * g / gs).  K / V is read from HBM once per KV head whenever g * sq <= 32, else g / gs times.
 *   ws: tf_attn_decode_ws_floats(cols, gs * sq, D, nsplit) floats; split count: tf_attn_decode_pick_nsplit(cols, sk);
 *   tickets: cols zeroed words = one launch (left zero), NULL = two launches; both bit-identical.  sk_dev as in
 *   tf_attn_decode_act.  K / V fp16.
 * tf_attn_prefill_gqa: tf_attn_prefill (utils/graph_infer.py:30-37 -> models/modeling_llama.py:240 with q_len = the chunk),
 *   1 <= sq <= 4096; split count and workspace from tf_attn_prefill_pick_nsplit / _ws_floats with H = the QUERY heads.
 * tf_skinny_qkv_rope_gqa_act: tf_skinny_qkv_rope_act (models/modeling_llama.py:213-224: q / k / v projections + RoPE, then
 *   the cache update of models/cache.py:50-61); weight rows [q: H D | k: Hkv D | v: Hkv D], N = (H + 2 Hkv) D, packed in
 *   triforce_amd.ops.rope_row_order(H, Hkv, D); q_out [M][H][D]; k / v rows to KV head hd of the Hkv-head cache.  Row-major
 *   x: xs_m = ld, xs_k = 8.
 * tf_rope_append_gqa: tf_rope_append for fused rows [q: H D | k: Hkv D | v: Hkv D] (the un-fused prefill-chunk path).
 * ------------------------------------------------------------------------------------------- */
int tf_attn_decode_gqa_act(const void* q, const void* k, const void* v, void* out, int64_t out_sm, int64_t out_sk,
                           int64_t stride_t, int64_t stride_h, int sq, int sk, const int32_t* sk_dev, int H, int Hkv, int D,
                           float scale, int nsplit, float* ws, int64_t ws_floats, uint32_t* tickets, void* stream);
int tf_attn_prefill_gqa(const void* q, const void* k, const void* v, void* out, int64_t stride_t, int64_t stride_h,
                        int sq, int sk, int H, int Hkv, int D, float scale, int nsplit, float* ws, int64_t ws_floats,
                        void* stream);
int tf_skinny_qkv_rope_gqa_act(const void* wqkv_packed, const void* x, int64_t xs_m, int64_t xs_k, const void* ln_w,
                               float eps, const float* ss_in, const void* cos, const void* sin, const int64_t* positions,
                               void* q_out, void* k_cache, void* v_cache, int64_t stride_t, int64_t stride_h, int slot0,
                               const int32_t* slot0_dev, int M, int H, int Hkv, int D, int K, int rotate_k, void* stream);
int tf_rope_append_gqa(const void* qkv, int64_t qkv_row_stride, const void* cos, const void* sin,
                       const int64_t* positions, void* q_out, void* k_cache, void* v_cache,
                       int64_t stride_t, int64_t stride_h, int slot0, const int32_t* slot0_dev,
                       int rows, int H, int Hkv, int D, int rotate_k, void* stream);

/* -------------------------------------------------------------------------------------------
 * QK NORM.  Qwen3-style targets normalise every q and k head over the head width before the rotation:
 * one [D] fp16 weight for all query heads (q_norm_w), one for all KV heads (k_norm_w), eps = the model's rms_norm_eps.
 * For one token row and one head, with x[0..D) the fp16 values of the q or k projection as the GEMM rounded them:
 *   ms   = (sum_d float(x[d])^2) / D          fp32; the sum in any order
 *   inv  = 1.0f / sqrtf(ms + eps)             fp32 (the expression of tf_rmsnorm)
 *   n[d] = fp16(float(x[d]) * inv)            cast BEFORE the weight multiply
 *   y[d] = hmul_rn(w[d], n[d])                fp16
 * — the rounding points of tf_rmsnorm (fp32 normalise -> fp16 -> times weight).  The fp16 rotation of tf_rope_append then
 * acts on y: hadd_rn(hmul_rn(y, cos), hmul_rn(rotate_half(y), sin)).
 * tf_qk_norm_rope_append: tf_rope_append_gqa with that norm in front of the rotation.  qkv rows [q: H D | k: Hkv D | v: Hkv D]
 *   fp16 at qkv + row * qkv_row_stride; q -> q_out[row][head][D]; k -> cache row slot0 + row (or *slot0_dev + row) of its KV
 *   head, normalised and, unless rotate_k == 0, rotated; v copied untouched.  Hkv == H is the multi-head case.  D = 64 or 128.
 *   TF_EINVAL: a NULL buffer, rows < 0, H or Hkv < 1, H % Hkv != 0, H > 65535, D outside {64, 128}, a norm weight that is not
 *   16-byte aligned, eps < 0 or NaN.  rows == 0 is a no-op after these gates.  One launch: one wave per (row, head), four
 *   waves per workgroup, no LDS, no workspace.
 * ------------------------------------------------------------------------------------------- */
int tf_qk_norm_rope_append(const void* qkv, int64_t qkv_row_stride, const void* cos, const void* sin,
                           const int64_t* positions, void* q_out, void* k_cache, void* v_cache,
                           int64_t stride_t, int64_t stride_h, int slot0, const int32_t* slot0_dev,
                           int rows, int H, int Hkv, int D, int rotate_k, const void* q_norm_w, const void* k_norm_w,
                           float eps, void* stream);

/* -------------------------------------------------------------------------------------------
 * PER-TOKEN LOG-PROBABILITIES.  For fp32 logits rows x[r] (row r at logits + r * row_stride,
 * row_stride >= V elements) and a target id per row:
 *   logprob[r] = x[r][t] - max_i x[r][i] - log sum_i exp(x[r][i] - max_i x[r][i]),   lse[r] = max + log sum
 * — the log-probability at temperature 1 with no top-k / top-p filter.  fp32 throughout, one workgroup per row, the row is
 * streamed in one pass (any V >= 1, any rows >= 1; no 32768 limit), 16-byte loads between the row's first and last 16-byte
 * boundary whatever base and stride are, a fixed summation order.  -inf entries are legal and carry mass 0; a -inf target
 * gives -inf; NaN entries and a row of -inf alone are outside the contract.  A target outside [0, V) means "no target":
 * logprob[r] = 0 and nothing is read for it.
 * tf_token_logprobs: targets is a DEVICE array of `rows` ids and may be NULL when only lse is wanted; lse may be NULL; at
 *   least one of (targets and logprob) or lse must be given.
 * tf_token_logprobs_ids: the ids (host memory, rows <= 32) travel as kernel arguments like tf_set_tokens' — the decode step
 *   knows them on the host and needs no upload; logprob is required, lse may be NULL.
 * TF_EINVAL before any launch: NULL logits, rows < 1, V < 1, row_stride < V, the output rule above (and rows > 32, NULL
 * host_ids / logprob for the _ids form).
 * ------------------------------------------------------------------------------------------- */
int tf_token_logprobs(const float* logits, int64_t row_stride, const int64_t* targets, int rows, int V, float* logprob,
                      float* lse, void* stream);
int tf_token_logprobs_ids(const float* logits, int64_t row_stride, const int64_t* host_ids, int rows, int V,
                          float* logprob, float* lse, void* stream);

/* -------------------------------------------------------------------------------------------
 * ATTENTION BIAS: the q / k / v / o projections of a model with `attention_bias` (the reference builds
 * them with bias=config.attention_bias, models/modeling_llama.py:174-177).  Each entry is its bias-free neighbour — same
 * operands, layouts, launch forms and gates — plus `bias`: fp16 [N], 8-byte aligned, in the ROW ORDER OF THE PACKED WEIGHT
 * (q|k|v: triforce_amd.ops.rope_row_order(H, Hkv, D); plain: natural).  The contract:
 *   - for an output element with fp32 accumulator acc (the COMPLETE K sum) and bias b:  y = fp16(acc + float(b)) — one
 *     rounding, to nearest even;
 *   - the other steps keep their rounding points: q and k rows — the fp16 RoPE arithmetic acts on y (the bias goes in BEFORE
 *     the rotation); v rows — y is stored; plain with resid — out = fp16(resid + y) in fp16 as in tf_skinny_gemm_act, and
 *     ss_out is taken from that sum;
 *   - in a K-split form the bias is added once, where the partial sums have been folded, never per share;
 *   - rows >= M are not written.
 * tf_skinny_gemm_bias_act: tf_skinny_gemm_act with fp16 output (o_proj; the un-fused q|k|v projection of a <= 32-row block).
 * tf_skinny_qkv_rope_bias_act / tf_skinny_qkv_rope_gqa_bias_act: tf_skinny_qkv_rope_act / tf_skinny_qkv_rope_gqa_act.
 * TF_EINVAL before any launch: NULL or misaligned bias, out_f32 != 0, and every gate of the neighbour.  The 8-row-panel and
 * the exchange forms (tensor-parallel shards) have no bias form.
 * ------------------------------------------------------------------------------------------- */
int tf_skinny_gemm_bias_act(const void* w_packed, const void* x, int64_t xs_m, int64_t xs_k, const void* ln_w, float eps,
                            const float* ss_in, const void* resid, int64_t rs_m, int64_t rs_k, float* ss_out, void* y,
                            int64_t ys_m, int64_t ys_k, int M, int N, int K, int out_f32, const void* bias, void* stream);
int tf_skinny_qkv_rope_bias_act(const void* wqkv_packed, const void* x, int64_t xs_m, int64_t xs_k, const void* ln_w,
                                float eps, const float* ss_in, const void* cos, const void* sin, const int64_t* positions,
                                void* q_out, void* k_cache, void* v_cache, int64_t stride_t, int64_t stride_h, int slot0,
                                const int32_t* slot0_dev, int M, int H, int D, int K, int rotate_k, const void* bias,
                                void* stream);
int tf_skinny_qkv_rope_gqa_bias_act(const void* wqkv_packed, const void* x, int64_t xs_m, int64_t xs_k, const void* ln_w,
                                    float eps, const float* ss_in, const void* cos, const void* sin,
                                    const int64_t* positions, void* q_out, void* k_cache, void* v_cache, int64_t stride_t,
                                    int64_t stride_h, int slot0, const int32_t* slot0_dev, int M, int H, int Hkv, int D,
                                    int K, int rotate_k, const void* bias, void* stream);

/* -------------------------------------------------------------------------------------------
 * SAMPLING PENALTIES: repetition, frequency and presence penalties on the target tier's fp32 logits.
 * State (device, V entries each): gen_count int32 — occurrences among the generated tokens of the current answer, the pending
 * token excluded; prompt_seen uint8 — 1 where the token occurs in the context the answer is conditioned on.
 * tf_penalize_logits: for row i of a block whose input tokens are ids[0 .. rows) (ids may be NULL: no tokens), entry t with
 * raw logit x = logits[i * ls_m + t]:
 *     c    = gen_count[t] + #{ j <= i : ids[j] == t }                       (int32)
 *     seen = prompt_seen[t] != 0 || c > 0
 *     y = x
 *     if seen && repetition != 1:  y = (x > 0) ? x / repetition : x * repetition
 *     if c > 0:                    y = y - frequency * (float)c ;  y = y - presence
 *     out[i * os_m + t] = y
 *   Every / * - is ONE IEEE fp32 operation with its own rounding (no contraction); an entry with !seen is copied bit for bit;
 *   -inf stays -inf; NaN and +inf are outside the contract.  An id outside [0, V) matches no entry.  One launch over V, a
 *   thread owns four entries for all rows; 16-byte loads / stores when V, ls_m and os_m are multiples of 4 and logits, out,
 *   gen_count are 16-byte (prompt_seen 4-byte) aligned, else a scalar path with the same results.  Only READS the state: no
 *   atomics, no workspace, nothing shared between workgroups — capturable, replayable back to back.  out == logits (exactly)
 *   is allowed; any other overlap is not.
 *   TF_EINVAL before any launch: NULL logits / out / gen_count / prompt_seen, rows outside [1, 64], V < 1, ls_m < V or
 *   os_m < V, repetition not finite or <= 0, frequency or presence not finite (negative values are legal).
 * tf_penalty_commit: gen_count[ids[j]] += 1 for j < n (device ids; duplicates accumulate; an id outside [0, V) is skipped,
 *   never written).  One small workgroup.  TF_EINVAL: NULL gen_count or ids (checked BEFORE n == 0), n outside [0, 64], V < 1;
 *   n == 0 is a no-op returning 0.
 * ------------------------------------------------------------------------------------------- */
int tf_penalize_logits(const float* logits, int64_t ls_m, float* out, int64_t os_m, const int64_t* ids,
                       const int32_t* gen_count, const uint8_t* prompt_seen, int rows, int V, float repetition,
                       float frequency, float presence, void* stream);
int tf_penalty_commit(int32_t* gen_count, const int64_t* ids, int n, int V, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N-GRAM DRAFT: prompt lookup — a draft tier without weights, at any vocabulary.
 * State (device): hist int32 [cap] — the confirmed tokens; len_dev int32 scalar L, read as clamp(L, 0, cap).
 * tf_ngram_draft: blk int64, first m entries used — the speculative block in front of the proposal.
 *     ctx = hist[0:L] ++ blk[0:m],  T = L + m
 *     for 0 <= j <= T - 2:  l(j) = the largest n <= min(N, j + 1) with ctx[j - k] == ctx[T - 1 - k] for all 0 <= k < n, else 0
 *     an id outside [0, V) equals nothing, itself included (an entry of blk outside int32 is such an id)
 *     j* maximises (l(j), j) lexicographically: the longest match first, the most recent among equals
 *     d = ctx[j* + 1] when l(j*) >= 1;  else (no match, or T == 1) d = ctx[T - 1];  d outside [0, V): d = 0
 *     q[v] = (v == d) ? 1.0f : 0.0f for every v < V, whatever q held;  info[0..4) = (d, l(j*), l(j*) >= 1 ? j* : -1, T)
 *   ONE launch of a fixed grid (thread t owns the candidates j of the groups of four 4 g .. 4 g + 3, g = t, t + threads, ...,
 *   read with 16-byte loads; the <= 31 candidates inside blk belong to workgroup 0).  tf_ngram_draft_shape writes the HOST
 *   array out[2] = (threads of the grid, bytes of ws); TF_EINVAL for NULL.
 *   ws: that many bytes, 8-byte aligned, zero when first used; every launch leaves it zero — no zeroing between
 *   launches, capturable, replayable back to back, no host read.  Launches that share a ws must be ordered (one stream).
 *   TF_EINVAL before any launch: a NULL pointer, cap < 1, m outside [1, 32], N outside [1, 8], V < 1, cap + m > INT32_MAX,
 *   hist not 16-byte, q not 4-byte or ws not 8-byte aligned.
 * tf_ngram_commit: hist[L + i] = (int32)src[i] for i < n, then L += n (device ids; one wave, outside every graph).  L < 0 or
 *   L + n > cap: nothing is written (the host checks the capacity first).  TF_EINVAL: NULL hist / len_dev / src (checked
 *   BEFORE n == 0), cap < 1, n outside [0, 64]; n == 0 is a no-op returning 0.
 * ------------------------------------------------------------------------------------------- */
int tf_ngram_draft_shape(int32_t* out);
int tf_ngram_draft(const int32_t* hist, int cap, const int32_t* len_dev, const int64_t* blk, int m, int N, int V, float* q,
                   int32_t* info, void* ws, void* stream);
int tf_ngram_commit(int32_t* hist, int cap, int32_t* len_dev, const int64_t* src, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIFORCE_HIP_H */
