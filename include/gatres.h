/*
 * gatres.h -- C-ABI of the MI355X (gfx950) GATRes message-passing engine.
 *
 * Drop-in boundary for ONE hot path of DiTEC-project/gnn-pressure-estimation: the
 * GATConv-with-residual stack `GATResMeanConv` (reference gnn_pressure_estimation/GraphModels.py:454-494),
 * forward + backward, and the training step around it (train.py:159-190).  The reference has no FFI of its
 * own for this path (it is pure Python over torch_geometric); these entry points are what a ctypes binding
 * on the reference side would call (INTEGRATION.md shows that binding).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - feature matrices are row-major fp32, [rows, cols] with cols contiguous;
 *   - graph index arrays are int32;
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it (no allocation, no
 *     synchronisation) so a caller may capture any sequence of calls into a hipGraph;
 *   - return value: 0 = ok; < 0 = argument error (GATRES_E_*); > 0 = hipError_t from the launch.
 *
 * Supported widths: the whole-network drivers (gatres_model_t) take nc (hidden channels) a power of two in [4, 128]
 * (gatres_small: 32, gatres_large: 128).  The per-op entry points state their own, wider, contract beside their
 * declarations: lin0 forward takes any multiple of 4, lin1 forward a power of two up to 256, the two lin backward calls
 * every width from 1 to 256.  A width outside an entry point's contract is refused with GATRES_E_UNSUPPORTED.
 */
#ifndef GATRES_H
#define GATRES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 9 also after gatres_stage_multi_rows_mask_required and gatres_gather_multi_rows were added: two new symbols, no existing
 * signature or struct changed, so a library of ABI 9 exists with and without them.  gatres_version()'s build id (a hash of
 * the sources) tells such libraries apart; _native.load() checks it. */
#define GATRES_ABI_VERSION 9

#define GATRES_E_BADARG      (-1)  /* null pointer, negative size, misaligned pointer            */
#define GATRES_E_UNSUPPORTED (-2)  /* width not supported by the gfx950 kernels                  */
#define GATRES_E_GRAPH       (-3)  /* edge endpoint out of range while building the graph plan   */

#define GATRES_DTYPE_F32  0        /* storage types of activation-sized tensors (gatres_model_t.act_dtype) */
#define GATRES_DTYPE_BF16 1

/* --------------------------------------------------------------------------------------------------------
 * Graph plan (K0).  Replaces what PyG re-derives inside every GATConv.forward call --
 * remove_self_loops + add_self_loops (torch_geometric.utils.loop; reference call sites
 * GraphModels.py:464-465) -- and the scatter indices of GATConv / SimpleConv (GraphModels.py:464-466).
 * Built once per topology.
 *   gat CSR   : edges of edge_index with src != dst, then one self loop per node appended (PyG order),
 *               stably sorted by destination.              rowptr[N+1], col[E'] = source node.
 *   gat CSR^T : the same edge list stably sorted by source. t_rowptr[N+1], t_eid[E'] = position of the
 *               edge in the destination-sorted list, t_dst[E'] = destination node.
 *   mean CSR  : the ORIGINAL edge_index (self loops kept, none added) sorted by destination (SimpleConv).
 *   mean CSR^T: sorted by source.  mt_dst[E] = destination node.
 * ------------------------------------------------------------------------------------------------------ */
typedef struct gatres_graph {
  int32_t num_nodes;        /* N                                         */
  int32_t num_edges_gat;    /* E' = #(src != dst) + N                    */
  int32_t num_edges_mean;   /* E  = edge_index.shape[1]                  */
  int32_t num_segments;     /* 0 = no segment table (per-op kernels only) */
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* t_rowptr;
  const int32_t* t_eid;
  const int32_t* t_dst;
  const int32_t* m_rowptr;
  const int32_t* m_col;
  const int32_t* mt_rowptr;
  const int32_t* mt_dst;
  /* Segments: contiguous node ranges [seg_ptr[s], seg_ptr[s+1]) that no edge leaves -- the snapshots of a PyG
   * Batch (train.py:302-303).  The fused kernels give each segment to one workgroup. */
  const int32_t* seg_ptr;   /* [num_segments + 1]                         */
  int32_t max_segment_nodes;
  int32_t max_segment_edges_gat;   /* most GATConv edges (self loops included) inside one segment */
  int32_t max_segment_edges_mean;  /* most SimpleConv edges inside one segment                    */
  int32_t flags;            /* GATRES_GRAPH_* bits from gatres_graph_flags_host (0 = nothing known)        */
  /* Row windows of split segments, from gatres_graph_windows_host: window[M - 2] = {rows, GATConv edges, SimpleConv
   * edges} for M = 2 .. 8 workgroups per segment.  All zero = unknown (the fused kernels then size their LDS tables by
   * the whole segment). */
  int32_t window[7][3];
  int32_t reserved2;
  /* Node relabelling of the plan (gatres_graph_reorder_host): every array above is built on the RELABELLED graph and
   * perm[new id] = the caller's node id.  Only the arrays the caller hands over or gets back -- x, y, mask, out, g_out,
   * g_x -- are indexed through it, inside lin0 / lin1 / the loss, so the nn.Module contract is unchanged.  NULL = identity.
   * A relabelling permutes nodes, never a row's edge list: inside a destination row the edges keep PyG's order, so every
   * fp32 sum associates exactly as without it. */
  const int32_t* perm;
  /* Split segments: the most edges one part has to a row of ANOTHER part (in- or out-edges of the GATConv graph, whichever
   * is more), halo[M - 2] for M = 2 .. 8 workgroups per segment; from gatres_graph_windows_host.  The window kernel keeps
   * its halo lists (one entry per such edge) in LDS and is only taken when they fit. */
  int32_t halo[7];
  int32_t reserved3;
  /* Part tables of split segments (gatres_graph_part_tables_host), for part_tables_m workgroups per segment: one record of
   * part_tables_stride int32 words per (segment, part), device memory.  NULL, or an m other than the one a launch uses: the
   * window kernel derives the same tables from the CSR arrays in its prologues (correct, ~15 us slower per launch). */
  const int32_t* part_tables;
  int32_t part_tables_m;
  int32_t part_tables_stride;
} gatres_graph_t;

/* Header words of one part-table record (the tables follow; offsets are in int32 words from the record's start) */
enum {
  GATRES_PT_MAGIC = 0, GATRES_PT_M, GATRES_PT_N0, GATRES_PT_N, GATRES_PT_E0, GATRES_PT_EM0, GATRES_PT_T0, GATRES_PT_MT0,
  GATRES_PT_LO, GATRES_PT_HI, GATRES_PT_WLO, GATRES_PT_WHI, GATRES_PT_ELO, GATRES_PT_OEG, GATRES_PT_EWLO, GATRES_PT_WEG,
  GATRES_PT_MELO, GATRES_PT_OEM, GATRES_PT_TLO, GATRES_PT_OTG, GATRES_PT_MTLO, GATRES_PT_OTM,
  GATRES_PT_F_IMG, GATRES_PT_F_IMG_WORDS, GATRES_PT_F_HLIST, GATRES_PT_F_HCNT, GATRES_PT_F_ELIST, GATRES_PT_F_ECNT,
  GATRES_PT_B_IMG, GATRES_PT_B_IMG_WORDS, GATRES_PT_B_HROW, GATRES_PT_B_HRCNT, GATRES_PT_B_HEDGE, GATRES_PT_B_HECNT,
  GATRES_PT_B_EROW, GATRES_PT_B_ERCNT, GATRES_PT_B_EEDGE, GATRES_PT_B_EECNT,
  GATRES_PT_HEADER = 48
};
#define GATRES_PT_MAGIC_VALUE 0x47545031

/* gatres_graph_t.flags */
#define GATRES_GRAPH_SYMMETRIC 1   /* every edge (u, v), u != v, has its reverse (v, u) in edge_index -- what
                                    * pgu.from_networkx gives for an undirected water network (utils/DataLoader.py:29).  The parts
                                    * of a split segment then owe each other halo rows in BOTH directions at every hand-off,
                                    * which paces them without the heartbeat granules (k_fused_dev.h: xch_heartbeat). */

#define GATRES_GRAPH_DEG_LE32 2    /* no node has more than 31 edges into it or out of it in edge_index: every row of the
                                    * plan's CSRs (GATConv's with its self loop, SimpleConv's, their transposes) has at most
                                    * 32 entries.  The blocked kernels (gatres_bf16_*_proj / _src_dx) walk a row with its own
                                    * lane group and are only taken for such plans; others keep the per-op kernels, whose hub
                                    * rows are reduced by whole waves. */

#define GATRES_GRAPH_DEG_LE6 4     /* no node has more than 5 edges into it or out of it in edge_index: every row of the plan's
                                    * CSRs has at most 6 entries (the per-snapshot kernels' slot width, MAXD).  The window kernel
                                    * then runs an instantiation without the edge-at-a-time paths of its stages (k_window.hip). */

/* Host-side plan builder (runs on the CPU, once per topology).  edge_index_host: int64 [2, E] row-major as
 * torch stores it.  Step 1: count -> E'.  Step 2: fill caller-allocated HOST arrays sized from that count. */
int gatres_graph_count_host(const int64_t* edge_index_host, int64_t num_edges, int64_t num_nodes,
                            int64_t* num_edges_gat_out);
int gatres_graph_build_host(const int64_t* edge_index_host, int64_t num_edges, int64_t num_nodes,
                            int32_t* rowptr, int32_t* col, int32_t* t_rowptr, int32_t* t_eid, int32_t* t_dst,
                            int32_t* m_rowptr, int32_t* m_col, int32_t* mt_rowptr, int32_t* mt_dst);

/* Properties of the edge list the kernels may rely on (host): *flags_out = OR of GATRES_GRAPH_* bits. */
int gatres_graph_flags_host(const int64_t* edge_index_host, int64_t num_edges, int64_t num_nodes, int32_t* flags_out);

/* Part tables (host): see gatres_graph_t.part_tables.  Inputs: the plan's HOST arrays (as gatres_graph_build_host filled
 * them) and its segment table; m = workgroups per segment (2 .. 8, gatres_fused_cus_per_segment).  Call once with
 * out = NULL to learn the record size (*stride_words_out, a multiple of 4), then with an array of
 * num_segments * m * stride words.
 * Contract.  The arrays' lengths are not passed, so the caller owes: seg_ptr holds num_segments + 1 entries, every row
 * pointer array reaches index seg_ptr[num_segments], and the column arrays reach the last row pointer.  Checked before
 * anything is written, in this order:
 *   GATRES_E_BADARG       a NULL array, seg_ptr or stride_words_out; num_segments <= 0; m outside 2 .. 8; a negative
 *                         stride_words with out != NULL; seg_ptr[0] < 0 or a seg_ptr that decreases; a row pointer array
 *                         that is negative at, or decreases over, a segment's rows;
 *   GATRES_E_GRAPH        a segment whose CSR and transposed CSR hold different edge counts;
 *   GATRES_E_UNSUPPORTED  a segment of more than 65535 nodes, GATConv edges or SimpleConv edges (16-bit tables);
 *   GATRES_E_GRAPH        a col / t_dst / m_col / mt_dst entry outside its row's segment, or a t_eid outside the
 *                         segment's GATConv edge range.
 * While filling: a record longer than stride_words returns GATRES_E_BADARG; the records before it have been written,
 * nothing at or beyond it.  Words of a record beyond its last list are written as zeros.
 * *stride_words_out is written on success only.  Empty segments and parts without rows are records like any other. */
int gatres_graph_part_tables_host(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_eid,
                                  const int32_t* t_dst, const int32_t* m_rowptr, const int32_t* m_col,
                                  const int32_t* mt_rowptr, const int32_t* mt_dst, const int32_t* seg_ptr,
                                  int32_t num_segments, int32_t m, int32_t* out, int64_t stride_words,
                                  int64_t* stride_words_out);

/* Segment table (host): the finest partition of [0, N) into contiguous ranges closed under the edges, adjacent
 * ranges merged while the result stays <= merge_upto nodes.  seg_ptr_host must hold N + 1 entries. */
int gatres_graph_segments_host(const int64_t* edge_index_host, int64_t num_edges, int64_t num_nodes,
                               int32_t merge_upto, int32_t* seg_ptr_host, int32_t* num_segments_out,
                               int32_t* max_segment_nodes_out, int32_t* max_segment_edges_gat_out,
                               int32_t* max_segment_edges_mean_out);

/* Row windows of split segments (see gatres_graph_t.window): for M = 2 .. 8 workgroups per segment, the largest
 * contiguous row range a part needs (own rows + the rows adjacent to them), in rows / GATConv edges / SimpleConv edges,
 * followed by gatres_graph_t.halo: out28 = {rows2, gat2, mean2, ..., rows8, gat8, mean8, halo2, ..., halo8}.
 * These figures size the LDS that gatres_graph_part_tables_host's records fill: for every m, no record's window has more
 * rows, GATConv edges or SimpleConv edges than window[m - 2], and no hand-off list more entries than halo[m - 2].
 * Contract, checked in this order before any index is formed: GATRES_E_BADARG for a NULL edge_index (with
 * num_edges > 0), seg_ptr or out28, num_edges < 0, num_nodes <= 0 or num_segments <= 0; GATRES_E_UNSUPPORTED for
 * num_nodes > INT32_MAX; GATRES_E_BADARG for a segment table that does not start at 0, decreases, or does not end at
 * num_nodes; GATRES_E_GRAPH for an endpoint outside [0, num_nodes) and for an edge that joins two segments.  out28 is
 * written on success only. */
int gatres_graph_windows_host(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes, const int32_t* seg_ptr,
                              int32_t num_segments, int32_t* out28);

/* Bandwidth-reducing relabelling (host): reverse Cuthill-McKee inside every segment (nodes never leave their segment, so
 * seg_ptr stays valid).  perm_new2old_host[new] = old, N entries.  The fused kernels' row windows (above) are what it
 * shrinks: real .inp junction orders are not locality-preserving (utils/DataLoader.py:28-37 keeps the file order).
 * The segment table is held to the contract of gatres_graph_windows_host (GATRES_E_BADARG); an endpoint out of range or
 * an edge that leaves its segment is GATRES_E_GRAPH. */
int gatres_graph_reorder_host(const int64_t* edge_index_host, int64_t num_edges, int64_t num_nodes,
                              const int32_t* seg_ptr_host, int32_t num_segments, int32_t* perm_new2old_host);

/* LZ4 block decompression on the host (the Blosc-lz4 chunks of the reference's zarr stores, utils/DataLoader.py:212-242).
 * Returns the number of bytes written to dst, or GATRES_E_BADARG on malformed input / a dst that is too small. */
int64_t gatres_lz4_decompress_host(const uint8_t* src, int64_t src_len, uint8_t* dst, int64_t dst_cap);

/* The library reads its GATRES_* tuning / fallback switches from the environment once, at first use, never on a launch
 * path.  A process that changes them afterwards calls this to have them read again.  Always returns 0. */
int gatres_knobs_reload(void);

/* 64-bit content hash of an int64 [2,E] DEVICE edge_index (for plan caching); hash_out: device uint64[1],
 * must be zeroed by the caller on the same stream before the call.  The call ADDS to hash_out, modulo 2^64, the sum over
 * the edges e of mix64(mix64(src_e + 0x9E3779B97F4A7C15 * (e + 1)) ^ (dst_e + 0xD1B54A32D192ED03)), mix64 being the
 * finaliser of splitmix64: it depends on every endpoint and on every edge's position, not on the order of the additions.
 * num_edges == 0: returns 0 and leaves hash_out untouched (edge_index may then be NULL). */
int gatres_edge_index_hash(const int64_t* edge_index, int64_t num_edges, uint64_t* hash_out, void* stream);

/* --------------------------------------------------------------------------------------------------------
 * Per-op kernels.  Each replaces the PyG op sequence named in its comment.
 * ------------------------------------------------------------------------------------------------------ */

/* lin0: PyG Linear(1, nc) (GraphModels.py:477,487).  out[n,c] = xm[n]*w[c] + b[c], where xm[n] = 0 if
 * mask != NULL and mask[n] != 0 (the caller-side `data.x[batch_mask] = 0`, train.py:174) -- whatever x[n] holds, NaN
 * included.  One fp32 product and one fp32 sum per element (no fused multiply-add).  nc: any multiple of 4, nc >= 4 (others:
 * GATRES_E_UNSUPPORTED); w, b and out 16-byte aligned (GATRES_E_BADARG). */
int gatres_lin0_fwd(const float* x, const uint8_t* mask, const float* w, const float* b, float* out,
                    int32_t num_nodes, int32_t nc, void* stream);

/* K1: GATConv's lin_src projection + attention logits (GATConv.forward:
 *   h = lin(x).view(N,H,C); a_src = (h*att_src).sum(-1); a_dst = (h*att_dst).sum(-1)).
 * fp32 MFMA (v_mfma_f32_16x16x4_f32).  W is [H*C, K] row-major (PyG Linear.weight). */
int gatres_proj_attn_fwd(const float* x, const float* W, const float* att_src, const float* att_dst,
                         float* h, float* a_src, float* a_dst,
                         int32_t num_nodes, int32_t K, int32_t H, int32_t C, void* stream);

/* K2: GATConv edge scoring + per-destination softmax + weighted neighbour sum + bias (+ReLU)
 * (GATConv.edge_update / torch_geometric.utils.softmax / message / aggregate; heads concatenated;
 * heads=1, concat=False is the H=1 case).  alpha[E',H] is written for the backward pass. */
int gatres_gat_aggregate_fwd(const gatres_graph_t* g, const float* h, const float* a_src, const float* a_dst,
                             const float* bias, float* out, float* alpha,
                             int32_t H, int32_t C, int32_t apply_relu, void* stream);

/* K3: SimpleConv(aggr="mean")(y) + x0, then ReLU (GraphModels.py:466-467). */
int gatres_mean_residual_relu_fwd(const gatres_graph_t* g, const float* y, const float* x0, float* out,
                                  int32_t C, void* stream);

/* lin1: PyG Linear(nc, 1) (GraphModels.py:484,492).  out[n] = sum_c x[n,c]*w[c] + b[0]; b == NULL adds nothing.
 * nc: a power of two, 4 <= nc <= 256 (others: GATRES_E_UNSUPPORTED); x and w 16-byte aligned (GATRES_E_BADARG).  A row's sum
 * does not depend on the row's position. */
int gatres_lin1_fwd(const float* x, const float* w, const float* b, float* out,
                    int32_t num_nodes, int32_t nc, void* stream);

/* ---- backward -------------------------------------------------------------------------------------- */

/* Gradient partial sums.  Every reduction over nodes is done by `num_slabs` waves, each writing its partial
 * into its own slab of a [num_slabs, slab_stride] fp32 buffer at the parameter's flat offset; a final
 * gatres_reduce_slabs sums the slabs in a fixed order (bitwise reproducible, no atomics): out[i] is the fp32 sum of
 * slabs[s * slab_stride + i], s = 0 .. num_slabs - 1 in that order, starting from +0.0f, for i < count.
 * slab_stride < count, count <= 0 or num_slabs <= 0: GATRES_E_BADARG.
 * Slab s of every such reduction holds the rows [s * nps, min(N, (s + 1) * nps)), nps = ceil(N / num_slabs) rounded up to a
 * multiple of 4; a slab without rows is written as +0.0f. */
int gatres_reduce_slabs(const float* slabs, int32_t num_slabs, int64_t slab_stride, int64_t count,
                        float* out, void* stream);

/* lin1 backward.  g_x[n,c] = g_out[n]*w[c] (one fp32 product), exactly 0 where relu_mask != 0 and x[n,c] is not > 0 (x is
 * the last block's post-ReLU output).  slab_w / slab_b: this parameter's position inside slab 0; slab s gets
 * slab_w[c] = sum g_out[n]*x[n,c] and slab_b[0] = sum g_out[n] over its rows.  nc: 1 <= nc <= 256 (others:
 * GATRES_E_UNSUPPORTED).  A power of two >= 4 with 16-byte aligned x and g_x takes 256 threads per slab, every other width or
 * alignment (and GATRES_LIN_BWD_WAVE=1) one wave per slab: the same sums in another order. */
int gatres_lin1_bwd(const float* g_out, const float* x, const float* w, float* g_x,
                    float* slab_w, float* slab_b, int32_t num_slabs, int64_t slab_stride,
                    int32_t num_nodes, int32_t nc, int32_t relu_mask, void* stream);

/* K3 backward.  g_pre is the gradient w.r.t. the block's pre-ReLU sum (already ReLU-masked by its producer);
 * g_y[j] = sum over out-edges (j->i) of g_pre[i] / max(indeg(i), 1). */
int gatres_mean_bwd(const gatres_graph_t* g, const float* g_pre, float* g_y, int32_t C, void* stream);

/* K2 backward, destination-major pass: softmax / LeakyReLU backward per in-edge.
 * g_e[E',H] (grad w.r.t. the raw score a_src[j]+a_dst[i]) and g_a_dst[N,H]. */
int gatres_gat_aggregate_bwd_dst(const gatres_graph_t* g, const float* g_out, const float* h,
                                 const float* alpha, const float* a_src, const float* a_dst,
                                 float* g_e, float* g_a_dst, int32_t H, int32_t C, void* stream);

/* K2 backward, source-major pass over CSR^T (atomics-free):
 * g_a_src[j,h] = sum_out-edges g_e;  g_h[j] = sum alpha_e*g_out[i] + g_a_src (x) att_src + g_a_dst (x) att_dst. */
int gatres_gat_aggregate_bwd_src(const gatres_graph_t* g, const float* g_out, const float* alpha,
                                 const float* g_e, const float* g_a_dst, const float* att_src,
                                 const float* att_dst, float* g_h, float* g_a_src,
                                 int32_t H, int32_t C, void* stream);

/* K1 backward, data gradient: g_x = g_h @ W (fp32 MFMA), W given TRANSPOSED as Wt[K, HC] row-major.
 * Optional fused epilogue: g_x = (g_x + resid) masked by (relu_ref > 0)  (resid / relu_ref may be NULL). */
int gatres_proj_bwd_dx(const float* g_h, const float* Wt, const float* resid, const float* relu_ref,
                       float* g_x, int32_t num_nodes, int32_t K, int32_t HC, void* stream);

/* K1 backward, weight gradient partials: slab[s][c*K+k] = sum over slab s's nodes of g_h[n,c]*x[n,k]. */
int gatres_proj_bwd_dw(const float* g_h, const float* x, float* slab_W, int32_t num_slabs,
                       int64_t slab_stride, int32_t num_nodes, int32_t K, int32_t HC, void* stream);

/* Column reductions of one GATConv: partials of g_att_src[h,c] = sum_n g_a_src[n,h]*h[n,h,c], g_att_dst likewise,
 * g_bias[hc] = sum_n g_out[n,hc]. */
int gatres_conv_param_grads(const float* h, const float* g_a_src, const float* g_a_dst, const float* g_out,
                            float* slab_att_src, float* slab_att_dst, float* slab_bias, int32_t num_slabs,
                            int64_t slab_stride, int32_t num_nodes, int32_t H, int32_t C, void* stream);

/* lin0 backward partials: g_w[c] = sum_n g[n,c]*xm[n], g_b[c] = sum_n g[n,c] (mask == NULL: xm = x).  nc: 1 <= nc <= 256
 * (others: GATRES_E_UNSUPPORTED); the two forms of lin1's backward, chosen by nc and by the alignment of g. */
int gatres_lin0_bwd(const float* g, const float* x, const uint8_t* mask, float* slab_w, float* slab_b,
                    int32_t num_slabs, int64_t slab_stride, int32_t num_nodes, int32_t nc, void* stream);

/* Relabelled plans (gatres_graph_t.perm), per-op path: dst[i] = src[perm[i]] (scatter == 0) or dst[perm[i]] = src[i],
 * i < num_nodes: plain copies, every bit pattern is kept.  perm must be a permutation of 0 .. num_nodes - 1. */
int gatres_permute_f32(const float* src, const int32_t* perm, float* dst, int32_t num_nodes, int32_t scatter,
                       void* stream);
int gatres_gather_u8(const uint8_t* src, const int32_t* perm, uint8_t* dst, int32_t num_nodes, void* stream);

/* out[c*rows + r] = in[r*cols + c] for every GATConv weight of the flat parameter vector (see layout below): wt holds per
 * block [W1^T : nc x 2nc][W2^T : 2nc x nc], 4 nc^2 floats.  num_blocks == 0 returns 0 and writes nothing; nc >= 1. */
int gatres_transpose_conv_weights(const float* params, float* wt, int32_t num_blocks, int32_t nc, void* stream);

/* ---- caller side of the step (train.py:174-188) ---------------------------------------------------- */

/* Per-graph random node mask with EXACTLY int(n_g*rate) ones per graph (utils/auxil.py:143-182), generated
 * on the device.  node_ptr[B+1]: node offsets of the graphs; step_counter: device uint64[1] (read; combined
 * with seed so a replayed hipGraph draws a fresh mask each step when the caller bumps the counter). */
int gatres_mask_generate(const int32_t* node_ptr, int32_t num_graphs, double mask_rate, uint64_t seed,
                         const uint64_t* step_counter, uint8_t* mask, void* stream);

/* The same sampler AND the staging of a device-resident batch in ONE launch: x_dst[0..N) = x_src (and y_dst = y_src when
 * both are given; x_src may equal x_dst: nothing is copied then).  What `collate + mask` of train.py:159-173 amounts to
 * once snapshots live on the device: one small kernel and one kernel boundary less per step than a copy followed by
 * gatres_mask_generate. */
int gatres_stage_batch_mask(const float* x_src, const float* y_src, float* x_dst, float* y_dst, int64_t num_nodes,
                            const int32_t* node_ptr, int32_t num_graphs, double mask_rate, uint64_t seed,
                            const uint64_t* step_counter, uint8_t* mask, void* stream);

/* The same with the batch COLLATED on the way (utils/DataLoader.py:191-204 + the PyG DataLoader of train.py:302-303 for a
 * static topology): data is the device-resident snapshot matrix [S][nodes_per_graph], rows[num_graphs] (device, int64) the
 * snapshots of this batch; x_dst[g * nodes_per_graph + v] = data[rows[g]][v] (and y_dst likewise when given: targets are
 * the inputs before masking, utils/auxil.py:84-98). */
int gatres_stage_rows_mask(const float* data, const int64_t* rows, int32_t nodes_per_graph, float* x_dst, float* y_dst,
                           const int32_t* node_ptr, int32_t num_graphs, double mask_rate, uint64_t seed,
                           const uint64_t* step_counter, uint8_t* mask, void* stream);

/* gatres_stage_rows_mask whose mask always holds the sensor nodes (utils/auxil.py:143-163 with required_idx, evaluation.py's
 * second pass): required[num_required] (device int32) are node indices INSIDE a graph, distinct, in [0, nodes_per_graph);
 * every graph masks exactly int(nodes_per_graph * mask_rate) nodes -- the required ones and a uniform subset without
 * replacement of the others.  num_required >= int(nodes_per_graph * mask_rate) is refused (GATRES_E_BADARG), as the
 * reference refuses a mask length <= 0.  num_required == 0 draws the same masks as gatres_stage_rows_mask. */
int gatres_stage_rows_mask_required(const float* data, const int64_t* rows, int32_t nodes_per_graph, float* x_dst, float* y_dst,
                                    const int32_t* node_ptr, int32_t num_graphs, double mask_rate, uint64_t seed,
                                    const uint64_t* step_counter, const int32_t* required, int32_t num_required, uint8_t* mask,
                                    void* stream);

/* gatres_stage_rows_mask's collation with the mask of a FIXED sensor layout (fine-tuning a model to the sensors it is deployed
 * with; new symbol only: the ABI version stays).  observed[num_observed] (device int32): the sensors' node indices inside a
 * graph, distinct, each in [0, nodes_per_graph) -- the caller's duty, as for required[].
 * Collation: x_dst[g * N + v] = data[rows[g] * N + v] at EVERY node (and y_dst likewise when given), N = nodes_per_graph: the
 * step zeroes masked inputs itself and its target is x.
 * Draws (all integer arithmetic modulo 2^64; mix64: the splitmix64 finaliser behind the sampler's keys):
 *   step = step_counter ? step_counter[0] : 0,   base = seed + 0x9E3779B97F4A7C15 * (step + 1),
 *   T_drop = (uint32_t)(sensor_dropout * 16777216.0),   T_share = (uint32_t)(layout_share * 16777216.0);
 *   graph g takes the LAYOUT mask iff (mix64(base + 0x94D049BB133111EB * (g + 1)) >> 40) < T_share, else the RANDOM mask.
 * Layout mask of graph g, n0 = node_ptr[g]: mask[n0 + v] = 0 iff v == observed[k] for some k and
 *   (mix64(base + 0xBF58476D1CE4E5B9 * (n0 + v + 1)) >> 40) >= T_drop  (the hash of the sampler's key of that node, before its
 *   truncation); every other node of the graph, and every dropped sensor, gets mask = 1.  A graph that loses all its sensors
 *   to the dropout is masked everywhere: allowed (its loss then is the all-hidden one).
 * Random mask of graph g: byte for byte what gatres_stage_rows_mask writes for that graph with the same
 *   (mask_rate, seed, step_counter, node_ptr).
 * One launch of the sampler's grid; every byte of mask and every float of x_dst (y_dst) of the batch is written exactly once,
 * with plain stores.  A pure function of the arguments and *step_counter: a replayed capture draws fresh masks as the counter
 * advances.  sensor_dropout 0 and layout_share 1 give the mask bytes of gatres_stage_observed (seed, step and mask_rate unused);
 * layout_share 0 gives gatres_stage_rows_mask.
 * GATRES_E_BADARG before any launch: data, rows, x_dst, node_ptr, observed or mask NULL; data == x_dst; num_graphs <= 0 or
 * nodes_per_graph <= 0; num_observed < 1 or > nodes_per_graph; sensor_dropout outside [0, 1); layout_share or mask_rate
 * outside [0, 1]. */
int gatres_stage_rows_mask_sensors(const float* data, const int64_t* rows, int32_t nodes_per_graph, float* x_dst, float* y_dst,
                                   const int32_t* node_ptr, int32_t num_graphs, const int32_t* observed, int32_t num_observed,
                                   double sensor_dropout, double layout_share, double mask_rate, uint64_t seed,
                                   const uint64_t* step_counter, uint8_t* mask, void* stream);

/* gatres_stage_rows_mask_sensors with MEASUREMENT NOISE on the readings the layout keeps (fine-tuning a model to noisy sensors;
 * new symbol only: the ABI version stays).  The kernel of gatres_stage_rows_mask_sensors compiled with the noise as one more
 * compile-time fact; its arguments, and
 *   sigma        device float[num_observed], >= 0, in the units of data
 *   noise_seed   any 64-bit value.
 * The mask: byte for byte that of gatres_stage_rows_mask_sensors with the same arguments -- the mode draw per graph, the dropout
 *   draw per sensor and the random-mode mask do not see the noise.
 * A RANDOM-mode graph is staged clean: x_dst and y_dst are the row.
 * A LAYOUT-mode graph g, n0 = node_ptr[g] = g * N, source row r = rows[g]: at every sensor k that KEEPS its reading (mask = 0)
 *   x_dst[n0 + observed[k]] = fp32(data[r * N + observed[k]] + fp32(sigma[k] * z))
 *   with z the draw of gatres_stage_observed_noisy's generator (below) for (seed = noise_seed, member = step, row = r, k), K =
 *   num_observed, step = step_counter ? step_counter[0] : 0 -- estimation.reading_noise(noise_seed, 1, S, K, member0=step)[r, 0, k]
 *   restates it, sensor_layout.sensor_layout_noise names it.  z depends on nothing else: not on the graph's place in the batch,
 *   the launch geometry or the dropout of other sensors.  sigma[k] == 0 stores the row's value itself.
 * Every other element of x_dst is the clean row, the dropped sensors (mask = 1) included; y_dst, when given and another buffer
 *   than x_dst, is the clean row everywhere.  The noise sits only where mask == 0, and the loss and the metrics read their target
 *   only where mask == 1: a step whose target buffer IS x_dst (y_dst NULL or == x_dst) trains on clean targets.
 * One launch of the same grid, plain stores, no atomics: in a layout-mode graph each of the graph's workgroups copies its own
 * slice of the row and, behind a workgroup barrier, stores the noisy values of that slice over its own copy, so every element
 * has one final writer.  Only lanes that hold a kept sensor draw.  A pure function of the arguments and *step_counter: every
 * step of a replayed capture draws its own noise.
 * GATRES_E_BADARG before any launch: whatever gatres_stage_rows_mask_sensors refuses, sigma == NULL, and a sigma that overlaps
 * x_dst, y_dst or mask. */
int gatres_stage_rows_mask_sensors_noisy(const float* data, const int64_t* rows, int32_t nodes_per_graph, float* x_dst,
                                         float* y_dst, const int32_t* node_ptr, int32_t num_graphs, const int32_t* observed,
                                         int32_t num_observed, double sensor_dropout, double layout_share, double mask_rate,
                                         uint64_t seed, const uint64_t* step_counter, uint8_t* mask, const float* sigma,
                                         uint64_t noise_seed, void* stream);

/* gatres_stage_rows_mask_required for a batch whose graphs come from SEVERAL snapshot matrices (one [S_k][N_k] matrix per
 * water network; utils/DataLoader.py:61-183 takes lists of networks): src_table[num_networks] (device) holds the matrices'
 * device addresses; graph g is row rows[g] (device, int64) of matrix net_of_graph[g] (device, int32), node_ptr[g + 1] -
 * node_ptr[g] floats wide -- the caller guarantees that this is the matrix's row length and that the row exists -- and goes
 * to x_dst + node_ptr[g] (and y_dst likewise when given).  Required nodes are a CSR per network: network k's sensor nodes
 * are req_idx[req_ptr[k] .. req_ptr[k + 1]) (device, int32; indices inside a graph, distinct, fewer than int(N_k * mask_rate));
 * req_ptr == NULL (then req_idx == NULL too): none.  The sampler and its keys (seed, step, node) are those of the entry
 * points above: with one network the call writes the x and the mask bytes of gatres_stage_rows_mask_required.  A graph whose
 * table entry is out of range or null is not copied. */
int gatres_stage_multi_rows_mask_required(const float* const* src_table, int32_t num_networks, const int32_t* net_of_graph,
                                          const int64_t* rows, const int32_t* node_ptr, int32_t num_graphs, float* x_dst,
                                          float* y_dst, double mask_rate, uint64_t seed, const uint64_t* step_counter,
                                          const int32_t* req_ptr, const int32_t* req_idx, uint8_t* mask, void* stream);

/* The gather of gatres_stage_multi_rows_mask_required alone, for num_batches batches of the same composition in ONE launch:
 * rows[num_batches * num_graphs]; graph g of batch b goes to dst + b * batch_stride + node_ptr[g] (batch_stride in floats).
 * An epoch's full batches laid out batch by batch in one buffer. */
int gatres_gather_multi_rows(const float* const* src_table, int32_t num_networks, const int32_t* net_of_graph,
                             const int64_t* rows, const int32_t* node_ptr, int32_t num_graphs, int32_t num_batches, float* dst,
                             int64_t batch_stride, void* stream);

/* Masked-metric moments of one batch (evaluation.get_metric_fn_collection + MSELoss, utils/auxil.py:101-140,185-203):
 * one record of GATRES_METRICS_RECORD doubles into table[slot] (slot += *cursor when cursor != NULL; the kernel then
 * advances *cursor by one, so a replayed capture writes consecutive slots; a slot outside [0, capacity) is not written).
 * out, y: scaled fp32 [num_nodes]; p = fp32(fp32(out * (float)scale) + (float)offset), t likewise from y, as torch rounds
 * `descale()`.  Record over the masked nodes:
 *   [0] M   [1] sum (out - y)^2 (scaled)   [2] sum |p - t|   [3] sum (p - t)^2   [4] sum p   [5] sum t
 *   [6] sum (p - pm)^2   [7] sum (t - tm)^2   [8] sum (p - pm)(t - tm)     (pm, tm: the means of p, t; a second pass)
 *   [9] #{|t| > 0.01f}   [10] sum over those of |t - p| / |t|   [11] #{|t - p| <= t * 0.1f}   [12..15] 0
 * One workgroup, fixed-order fp64 reduction: the same bits on every run. */
#define GATRES_METRICS_RECORD 16
int gatres_masked_metrics(const float* out, const float* y, const uint8_t* mask, int32_t num_nodes, double scale,
                          double offset, double* table, int32_t slot, int32_t capacity, uint64_t* cursor, void* stream);

/* MSELoss(mean) over masked nodes + its gradient: loss[0] = mean_{mask}(out-y)^2, g_out[n] = mask ? 2(out-y)/M : 0. */
int gatres_masked_mse(const float* out, const float* y, const uint8_t* mask, float* loss, float* g_out,
                      int32_t num_nodes, void* stream);

/* Training criteria of the reference (train.py --criterion), over the M masked nodes, d = out - y:
 *   GATRES_LOSS_MSE  nn.MSELoss():  loss = sum d^2 / M,   g_out = 2 d / M
 *   GATRES_LOSS_MAE  nn.L1Loss():   loss = sum |d| / M,   g_out = sign(d) / M  (sign(0) = 0)
 *   GATRES_LOSS_SCE  sce_loss(alpha=3) of F.normalize(., dim=-1) on [M, 1] tensors, eps = 1e-12:
 *                    o^ = out / max(|out|, eps), y^ = y / max(|y|, eps), t = 1 - o^ y^;  loss = sum t^3 / M,
 *                    g_out = |out| < eps ? -3 t^2 y^ / (eps M) : 0  (o^ is +-1 elsewhere: the gradient is zero there)
 * Unmasked nodes get g_out = 0; M == 0 gives loss NaN and g_out = 0. */
#define GATRES_LOSS_MSE 0
#define GATRES_LOSS_MAE 1
#define GATRES_LOSS_SCE 2
/* The loss of `criterion` over the masked nodes and its gradient (GATRES_LOSS_MSE: the same bits as gatres_masked_mse). */
int gatres_masked_loss(const float* out, const float* y, const uint8_t* mask, int32_t criterion, float* loss, float* g_out,
                       int32_t num_nodes, void* stream);

/* torch.optim.Adam step (weight_decay folded into the gradient), step counter on the device:
 * step_counter is device uint64[2] = {step, internal ticket (must start at 0)}; the kernel uses step+1 for the
 * bias corrections and then increments step.  grad_scale multiplies the gradient first (1/world_size). */
int gatres_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                     uint64_t* step_counter, int64_t count, double lr, double beta1, double beta2, double eps,
                     double weight_decay, float grad_scale, void* stream);

/* --------------------------------------------------------------------------------------------------------
 * Typed per-op kernels: the per-op kernels above with the storage type of the activation-sized tensors as an argument
 * (`dtype`: GATRES_DTYPE_F32 or GATRES_DTYPE_BF16, defined with gatres_model_t below).  `void*` arguments are the tensors
 * whose element type `dtype` selects; every other pointer is fp32 / int32 exactly as in the fp32 entry point of the same
 * name, which is the GATRES_DTYPE_F32 instance.  bf16: loads widen to fp32, sums / softmax / accumulators stay fp32,
 * stores round to nearest-even; the projections run on v_mfma_f32_16x16x32_bf16 and need nc >= 32.
 * ------------------------------------------------------------------------------------------------------ */
/* k_aggregate.hip */
int gatres_t_gat_aggregate_fwd(const gatres_graph_t* g, const void* h, const float* a_src, const float* a_dst,
                               const float* bias, void* out, float* alpha, int H, int C, int apply_relu, int dtype,
                               void* stream);
int gatres_t_gat_aggregate_bwd_dst(const gatres_graph_t* g, const void* g_out, const void* h, const float* alpha,
                                   const float* a_src, const float* a_dst, float* g_e, float* g_a_dst, int H, int C,
                                   int dtype, void* stream);
int gatres_t_gat_aggregate_bwd_src(const gatres_graph_t* g, const void* g_out, const float* alpha, const float* g_e,
                                   const float* g_a_dst, const float* att_src, const float* att_dst, void* g_h,
                                   float* g_a_src, int H, int C, int dtype, void* stream);
int gatres_t_mean_residual_relu_fwd(const gatres_graph_t* g, const void* y, const void* x0, void* out, int C, int dtype,
                                    void* stream);
int gatres_t_mean_bwd(const gatres_graph_t* g, const void* g_pre, void* g_y, int C, int dtype, void* stream);

/* k_misc.hip.  Widths and alignments as stated at the fp32 entry points above: lin0 forward any multiple of 4, lin1 forward a
 * power of two up to 256, both backward calls 1 .. 256 (bf16 tables included: a bf16 activation one element off a 16-byte
 * boundary takes the one-wave form like an fp32 one). */
int gatres_t_lin0_fwd(const float* x, const uint8_t* mask, const float* w, const float* b, void* out, int num_nodes, int nc,
                      int dtype, void* stream);
int gatres_t_lin0_bwd(const void* g, const float* x, const uint8_t* mask, float* slab_w, float* slab_b, int num_slabs,
                      int64_t slab_stride, int num_nodes, int nc, int dtype, void* stream);
int gatres_t_lin1_fwd(const void* x, const float* w, const float* b, float* out, int num_nodes, int nc, int dtype,
                      void* stream);
int gatres_t_lin1_bwd(const float* g_out, const void* x, const float* w, void* g_x, float* slab_w, float* slab_b,
                      int num_slabs, int64_t slab_stride, int num_nodes, int nc, int relu_mask, int dtype, void* stream);
int gatres_t_conv_param_grads(const void* h, const float* g_a_src, const float* g_a_dst, const void* g_out,
                              float* slab_att_src, float* slab_att_dst, float* slab_bias, int num_slabs,
                              int64_t slab_stride, int num_nodes, int H, int C, int dtype, void* stream);
/* A convolution's parameter-gradient partials as the per-op backward launches them (model_driver.hip): the weight
 * partials (gatres_t_proj_bwd_dw) and the attention-vector / bias column sums (gatres_t_conv_param_grads) as ONE launch where
 * a co-launching kernel applies, else one after the other.  w_slabs: slab rows the weight partials use (== num_slabs, or
 * fewer for the two-dimensional partials of wide bf16 models). */
int gatres_t_conv_partials(const void* g_h, const void* x, float* slab_W, int w_slabs, int64_t slab_stride, int num_nodes,
                           int K, int HC, const void* h, const float* g_a_src, const float* g_a_dst, const void* g_out,
                           float* slab_att_src, float* slab_att_dst, float* slab_bias, int num_slabs, int H, int C, int dtype,
                           void* stream);
/* bf16 copies of every GATConv weight and of its transpose: wb block layout [W1 : 2nc x nc][W2 : nc x 2nc] */
/* [W1^T : nc x 2nc][W2^T : 2nc x nc] (4 * 2nc^2 bf16 per block), each element rounded to nearest-even.  num_blocks == 0 */
/* returns 0 and writes nothing; nc >= 1. */
int gatres_convert_conv_weights_bf16(const float* params, void* wb, int num_blocks, int nc, void* stream);

/* k_proj.hip.  W / Wt: fp32 for GATRES_DTYPE_F32, bf16 (from gatres_convert_conv_weights_bf16) for GATRES_DTYPE_BF16. */
int gatres_t_proj_attn_fwd(const void* x, const void* W, const float* att_src, const float* att_dst, void* h, float* a_src,
                           float* a_dst, int num_nodes, int K, int H, int C, int dtype, void* stream);
int gatres_t_proj_bwd_dx(const void* g_h, const void* Wt, const void* resid, const void* relu_ref, void* g_x, int num_nodes,
                         int K, int HC, int dtype, void* stream);
int gatres_t_proj_bwd_dw(const void* g_h, const void* x, float* slab_W, int num_slabs, int64_t slab_stride, int num_nodes,
                         int K, int HC, int dtype, void* stream);

/* --------------------------------------------------------------------------------------------------------
 * Whole-network drivers: enqueue every kernel of GATResMeanConv.forward / its backward natively.
 *
 * Flat parameter layout (fp32, state_dict order; GraphModels.py:472-484, :455-460):
 *   lin0.weight[nc]  lin0.bias[nc]
 *   per block: conv1.att_src[2nc] conv1.att_dst[2nc] conv1.bias[2nc] conv1.lin.weight[2nc, nc]
 *              conv2.att_src[nc]  conv2.att_dst[nc]  conv2.bias[nc]  conv2.lin.weight[nc, 2nc]
 *   lin1.weight[nc]  lin1.bias[1]
 * ------------------------------------------------------------------------------------------------------ */
typedef struct gatres_model {
  int32_t num_blocks;
  int32_t nc;
  /* Storage type of the activation-sized tensors between kernels (saved activations, their gradients) and operand type of
   * the projections' MFMAs.  GATRES_DTYPE_F32: exact fp32 everywhere (the 1e-5 parity path).  GATRES_DTYPE_BF16 (BASELINE
   * config 3): bf16 in HBM, v_mfma_f32_16x16x32_bf16 for lin(x) and its data gradient with fp32 accumulation; attention
   * logits, softmax, every neighbour sum, parameter gradients, master weights and Adam stay fp32.  Per-op kernels only
   * (the fused per-snapshot path is fp32).  Buffers keep their fp32 SIZES (gatres_saved_floats / gatres_scratch_floats):
   * a bf16 tensor occupies the first half of its fp32 slot.  x, y, out, g_out, g_x, params, grads are always fp32. */
  int32_t act_dtype;
  int32_t flags;            /* GATRES_MODEL_* bits (0 = none) */
} gatres_model_t;

/* gatres_model_t.flags */
#define GATRES_MODEL_INFERENCE 1   /* forward-only calls whose `saved` buffer nobody will read (evaluation): the per-snapshot
                                    * kernel still needs the buffer (pass gatres_saved_floats floats) but may leave it unwritten --
                                    * the window kernel then runs an instantiation without the saved-activation stores */

/* --------------------------------------------------------------------------------------------------------
 * Blocked kernels (round 5; k_blocked.hip): a SPARSE stage and the dense projection that consumes its output
 * as ONE launch -- bf16 storage, nc = 128 (gatres_large: ConfigModels.py:22-32; block GraphModels.py:462-468),
 * plans flagged GATRES_GRAPH_DEG_LE32.  A 512-thread workgroup aggregates a block of 32 rows (the arithmetic
 * of the gatres_t_* sparse kernels, statement for statement), stores them (later launches read them) and runs
 * them through the matrix cores from LDS against W fragments held in registers.  Each call gives what the two
 * per-op calls it replaces give (the next convolution's attention logits are summed in another order).
 *   gatres_blocked_supported   1 when gatres_model_forward/backward_per_op take these kernels for (m, g)
 *   gatres_bf16_agg_proj_fwd   = gatres_t_gat_aggregate_fwd(H = 2, ReLU) + gatres_t_proj_attn_fwd(K = 2nc, H = 1)
 *   gatres_bf16_mean_proj_fwd  = gatres_t_mean_residual_relu_fwd + gatres_t_proj_attn_fwd(K = nc, H = 2)
 *   gatres_bf16_src_dx_bwd     = gatres_t_gat_aggregate_bwd_src(H) + gatres_t_proj_bwd_dx
 * W_next / Wt: bf16 [M, K] row-major as gatres_convert_conv_weights_bf16 leaves them. */
int gatres_blocked_supported(const gatres_model_t* m, const gatres_graph_t* g);
int gatres_bf16_agg_proj_fwd(const gatres_graph_t* g, const void* h, const float* a_src, const float* a_dst,
                             const float* bias, void* o, float* alpha, const void* W_next, const float* att_src_next,
                             const float* att_dst_next, void* h_next, float* a_src_next, float* a_dst_next, int32_t nc,
                             void* stream);
int gatres_bf16_mean_proj_fwd(const gatres_graph_t* g, const void* y, const void* x0, void* x_next, const void* W_next,
                              const float* att_src_next, const float* att_dst_next, void* h_next, float* a_src_next,
                              float* a_dst_next, int32_t nc, void* stream);
int gatres_bf16_src_dx_bwd(const gatres_graph_t* g, const void* g_out, const float* alpha, const float* g_e,
                           const float* g_a_dst, const float* att_src, const float* att_dst, void* g_h, float* g_a_src,
                           const void* Wt, const void* resid, const void* relu_ref, void* g_x, int32_t H, int32_t nc,
                           void* stream);

int64_t gatres_param_count(int32_t num_blocks, int32_t nc);
/* floats of forward state kept for backward / of scratch needed by forward+backward / slabs used. */
int64_t gatres_saved_floats(const gatres_model_t* m, const gatres_graph_t* g);
int64_t gatres_scratch_floats(const gatres_model_t* m, const gatres_graph_t* g);
int32_t gatres_num_slabs(const gatres_model_t* m, int32_t num_nodes);

/* out[N] = GATResMeanConv(x).  saved == NULL: inference (activations are not kept; scratch is reused per block). */
int gatres_model_forward(const gatres_model_t* m, const gatres_graph_t* g, const float* params,
                         const float* x, const uint8_t* mask, float* out, float* saved, float* scratch,
                         void* stream);

/* grads[P] = d loss / d params given g_out[N] = d loss / d out; g_x (may be NULL) = d loss / d x. */
int gatres_model_backward(const gatres_model_t* m, const gatres_graph_t* g, const float* params,
                          const float* x, const uint8_t* mask, const float* g_out, const float* saved,
                          float* scratch, float* grads, float* g_x, void* stream);

/* The same two entry points restricted to the per-op kernels above (any graph, any segment size). */
int gatres_model_forward_per_op(const gatres_model_t* m, const gatres_graph_t* g, const float* params,
                                const float* x, const uint8_t* mask, float* out, float* saved, float* scratch,
                                void* stream);
int gatres_model_backward_per_op(const gatres_model_t* m, const gatres_graph_t* g, const float* params,
                                 const float* x, const uint8_t* mask, const float* g_out, const float* saved,
                                 float* scratch, float* grads, float* g_x, void* stream);

/* One piece of gatres_model_backward_per_op: [lin1 backward] + blocks b_hi-1 .. b_lo + [lin0 backward].  FIRST must
 * come with b_hi == num_blocks, LAST with b_lo == 0; pieces are issued in that order on one stream.  With REDUCE the
 * piece ends by summing its slab partials into grads[lo, hi), lo = LAST ? 0 : 2nc + b_lo*(9nc + 4nc^2),
 * hi = FIRST ? P : 2nc + b_hi*(9nc + 4nc^2) -- final values, so a data-parallel caller can start the all-reduce of that
 * range while the next piece runs (gradient buckets in reverse block order).  Without REDUCE nothing is summed and the
 * slab partials stay in scratch in a layout private to the engine (wide bf16 models keep fewer rows for the weight
 * matrices than for the other parameters): gatres_model_reduce_grads sums them after the LAST piece, as
 * gatres_model_backward_per_op does. */
#define GATRES_PART_FIRST  1
#define GATRES_PART_LAST   2
#define GATRES_PART_REDUCE 4
int gatres_model_backward_per_op_part(const gatres_model_t* m, const gatres_graph_t* g, const float* params,
                                      const float* x, const uint8_t* mask, const float* g_out, const float* saved,
                                      float* scratch, float* grads, float* g_x, int32_t b_hi, int32_t b_lo,
                                      int32_t flags, void* stream);

/* grads[0, P) = the sum of the per-op backward's slab partials in scratch (fixed order, bitwise reproducible). */
int gatres_model_reduce_grads(const gatres_model_t* m, const gatres_graph_t* g, float* scratch, float* grads, void* stream);

/* --------------------------------------------------------------------------------------------------------
 * Fused per-snapshot path (k_fused.hip): ONE launch carries every segment through the selected phases --
 * GATRES_PHASE_FORWARD (lin0 .. lin1), GATRES_PHASE_LOSS (masked MSE + d loss/d out; needs mask, y) and
 * GATRES_PHASE_BACKWARD (all gradients, as per-segment slabs in scratch) -- one workgroup per segment, neighbour
 * gathers of the forward pass served from LDS when a segment fits (C-Town at nc=32 does).  The backward phase
 * leaves the GATConv weight / attention-vector gradients to gatres_fused_param_grads (they are off the backward's
 * dependency chain: one workgroup per (segment, block, conv) over the kept g_h tables in scratch), which must run
 * between gatres_fused_run(BACKWARD) and gatres_fused_finish.  gatres_fused_finish
 * sums the slabs into grads[P] and optionally applies Adam and finalises the loss in the same pass.
 * gatres_model_forward/backward and gatres_train_step take this path whenever gatres_fused_supported().
 * A segment may be carried by up to 8 workgroups on 8 CUs (hand-offs through scratch; the split is chosen so
 * that the whole grid is resident; environment GATRES_FUSED_SPLIT=1..8 sets it).  The barrier epochs persist
 * in `scratch` from launch to launch: ZERO the scratch buffer once after allocating it and do not share it between
 * streams.  A partner that never arrives (e.g. the GPU is shared and the grid is not resident) turns out[first node
 * of the segment] / the lin1 bias gradient into NaN instead of hanging.
 * loss_part: device float[8 * num_segments + 1].  GATRES_PHASE_BACKWARD reads the transposed conv weights from scratch:
 * call gatres_fused_prepare_backward (one small launch) after the parameters last changed.
 * ------------------------------------------------------------------------------------------------------ */
#define GATRES_PHASE_LOSS 16
/* Qualifiers of GATRES_PHASE_LOSS in gatres_fused_run's `phases`: the loss phase forms that criterion's loss and gradient
 * (GATRES_LOSS_MAE / GATRES_LOSS_SCE, see gatres_masked_loss) instead of the masked MSE.  At most one; only with
 * GATRES_PHASE_LOSS (else GATRES_E_BADARG). */
#define GATRES_PHASE_LOSS_MAE 32
#define GATRES_PHASE_LOSS_SCE 64
int gatres_fused_supported(const gatres_model_t* m, const gatres_graph_t* g);
/* Workgroups (CUs) that carry one segment in the fused launches (1, 2, 4 or 8); 0 if the fused path is unavailable. */
int gatres_fused_cus_per_segment(const gatres_model_t* m, const gatres_graph_t* g);
/* 1 if launches that are given a `saved` buffer take the window kernel (LDS tables sized by the parts' row windows,
 * gatres_graph_t.window).  It is faster than the whole-segment-table kernel even for inference, so a caller that only
 * wants predictions may pass a throw-away `saved` buffer of gatres_saved_floats() to gatres_model_forward. */
int gatres_fused_window_kernel(const gatres_model_t* m, const gatres_graph_t* g);
/* What gatres_fused_run launches for this model, plan and `phases` (its argument) when it is given a `saved` buffer: the
 * decision function the launch itself calls, so the answer is the launch.  (Without a `saved` buffer a launch never takes
 * the window kernel; nothing else changes.)  num_cus <= 0: the current device's CUs; a positive value stands in for them in
 * this call only, so the decision for a full MI355X (256) can be asked for anywhere.  out[GATRES_FUSED_PLAN_WORDS]:
 *   PARTS       workgroups (CUs) per segment, gatres_fused_cus_per_segment
 *   WINDOW      1: the window kernel (LDS tables sized by the parts' row windows); 0: the whole-segment-table kernel
 *   CACHED      1: the whole-segment kernel keeps its gathered tables in LDS; 0: in global scratch (read when WINDOW == 0)
 *   KEEP        1: a forward + backward launch of the window kernel keeps ReLU masks and own-row g_pre in LDS
 *   FACTS       the launch facts that select the window kernel's instantiation: 0x400 rows of at most six entries,
 *               0x1000 parts of at most 64 own rows, 0x2000 inference (GATRES_MODEL_INFERENCE, forward only), 0x4000 probed
 *               dispatch (gatres_probe_xcd_dispatch)
 *   LAUNCHES    kernel launches (more than one when the whole grid would not be resident: rounds)
 *   PER_LAUNCH  segments per launch (the last launch takes what is left)
 *   GRID        workgroups of the first launch
 *   THREADS     threads per workgroup
 *   PART_ROWS   own rows of the largest part, 16 * ceil(tiles / PARTS)
 *   CUS         the CU count the decision was taken for
 * Returns 0; GATRES_E_UNSUPPORTED (out zeroed) where gatres_fused_supported() is 0: the per-op path takes the model. */
#define GATRES_FUSED_PLAN_PARTS 0
#define GATRES_FUSED_PLAN_WINDOW 1
#define GATRES_FUSED_PLAN_CACHED 2
#define GATRES_FUSED_PLAN_KEEP 3
#define GATRES_FUSED_PLAN_FACTS 4
#define GATRES_FUSED_PLAN_LAUNCHES 5
#define GATRES_FUSED_PLAN_PER_LAUNCH 6
#define GATRES_FUSED_PLAN_GRID 7
#define GATRES_FUSED_PLAN_THREADS 8
#define GATRES_FUSED_PLAN_PART_ROWS 9
#define GATRES_FUSED_PLAN_CUS 10
#define GATRES_FUSED_PLAN_WORDS 12
int gatres_fused_plan(const gatres_model_t* m, const gatres_graph_t* g, int32_t phases, int32_t num_cus, int32_t* out);
/* Zero the split-segment barrier state inside `scratch` (as in a freshly zeroed buffer).  Only needed after an aborted
 * launch or when the buffer comes from elsewhere; not inside a captured graph that also holds fused launches. */
int gatres_fused_reset_sync(const gatres_model_t* m, const gatres_graph_t* g, float* scratch, void* stream);
/* Two split launches must not run concurrently on one device (each needs its whole grid resident).  gatres_fused_run
 * orders itself behind the previous split launch when the stream changes; a captured launch cannot do that, so call
 * this on `stream` before REPLAYING a hipGraph that contains fused launches. */
int gatres_fused_serialize(void* stream);
/* How does the current device place the workgroups of a launch?  Runs ONCE per device (a 1-KB allocation, one launch of one
 * workgroup per CU, a synchronisation of `stream`: NOT inside a stream capture -- it then returns what is cached, 0 if nothing)
 * and caches: 1 = workgroups whose ids are 8 apart run on the same XCD (round-robin dispatch: every full MI355X), 0 = not.
 * With 1 the parts of a split segment take their shared L2 for granted and the launch starts WITHOUT its first cross-CU
 * barrier (round 6: 7 us per launch; every part still records its XCD id and compares at the end of the launch -- a mismatch
 * faults the launch, which is then dropped and counted like any other fault).  A caller that never asks gets the barrier. */
int gatres_probe_xcd_dispatch(void* stream);
/* Float index inside `scratch` of the split-launch status words {uint32 fault (set by a launch whose partner never
 * arrived; cleared by gatres_fused_finish / the next forward launch's epilogue), uint32 faults seen so far, uint32
 * internal}; -1 if the fused path does not apply.  A faulted training step is dropped: loss = NaN, gradients = NaN,
 * no Adam update, no step count. */
int64_t gatres_fused_status_offset(const gatres_model_t* m, const gatres_graph_t* g);
/* Diagnostic only: per-stage wall-clock stamps (100 MHz) of segment 0 for the following fused launches. */
int gatres_fused_set_stamps(uint64_t* stamps, int32_t capacity);
int gatres_fused_prepare_backward(const gatres_model_t* m, const gatres_graph_t* g, const float* params,
                                  float* scratch, void* stream);
int gatres_fused_run(const gatres_model_t* m, const gatres_graph_t* g, const float* params, const float* x,
                     const uint8_t* mask, const float* y, float* out, float* g_out, float* loss_part, float* g_x,
                     float* saved, float* scratch, int32_t phases, void* stream);
int gatres_fused_param_grads(const gatres_model_t* m, const gatres_graph_t* g, const float* saved, float* scratch,
                             void* stream);
int gatres_fused_finish(const gatres_model_t* m, const gatres_graph_t* g, float* scratch, float* grads,
                        const float* loss_part, float* loss, int32_t do_adam, float* params, float* exp_avg,
                        float* exp_avg_sq, uint64_t* step_counter, double lr, double beta1, double beta2,
                        double eps, double weight_decay, float grad_scale, void* stream);
/* The same with the hyper-parameters read from `hparams` (device double[5] {lr, beta1, beta2, eps, weight_decay}) when it
 * is not NULL. */
int gatres_fused_finish_hp(const gatres_model_t* m, const gatres_graph_t* g, float* scratch, float* grads,
                           const float* loss_part, float* loss, int32_t do_adam, float* params, float* exp_avg,
                           float* exp_avg_sq, uint64_t* step_counter, double lr, double beta1, double beta2,
                           double eps, double weight_decay, const double* hparams, float grad_scale,
                           const int32_t* mask_node_ptr, int32_t mask_graphs, double mask_rate, uint64_t mask_seed,
                           uint8_t* mask_next, void* stream);
/* mask_* : reserved for gatres_train_step's own sequence (GATRES_FLAG_MASK_NEXT: extra workgroups of the update launch sample
 * the device mask of the NEXT step -- what gatres_mask_generate would produce when called after this update); through this
 * entry point pass NULL / 0 (a non-NULL mask_next is refused with GATRES_E_UNSUPPORTED: the sampling tail reads a snapshot
 * that only the train step's parameter-gradient launch writes). */
/* gatres_fused_param_grads + gatres_fused_finish as ONE launch, for blocks [block_lo, block_hi) of the model (the whole
 * model: 0, num_blocks): every (block, conv) column's last workgroup sums the column's slab rows, writes grads and (do_adam)
 * applies Adam to those parameters; lin0's gradient rides on block 0, lin1's on the last block, so the ranges
 * [0, p(block_hi)) ... tile the flat vector like gatres_model_backward_per_op_part's.  do_adam needs the whole model in one
 * call.  Returns GATRES_E_UNSUPPORTED where the two-launch form has to be used (nc other than 16 / 32). */
/* 1 if gatres_fused_param_grads_finish applies to this model / plan (else it returns GATRES_E_UNSUPPORTED). */
int gatres_fused_finish_folds(const gatres_model_t* m, const gatres_graph_t* g);
int gatres_fused_param_grads_finish(const gatres_model_t* m, const gatres_graph_t* g, const float* saved, float* scratch,
                                    float* grads, const float* loss_part, float* loss, int32_t do_adam, float* params,
                                    float* exp_avg, float* exp_avg_sq, uint64_t* step_counter, double lr, double beta1,
                                    double beta2, double eps, double weight_decay, const double* hparams,
                                    float grad_scale, int32_t block_lo, int32_t block_hi, void* stream);

/* --------------------------------------------------------------------------------------------------------
 * AutoClip gradient-norm clipping (reference utils/gradient_clipping.py; train.py:186-187 with
 * --use_gradient_clipping True --percentile p).  Per update, with g = grads * grad_scale (the gradient Adam sees, before
 * weight decay):
 *   n = ||g||_2 (fp64 sum of squares of the fp32 values, summed in a fixed order);  the history gets n appended;
 *   c = np.percentile(history, percentile) (numpy's default "linear" method, the current norm included);
 *   coef = min(1, c / (n + 1e-6)) (torch.nn.utils.clip_grad_norm_: ALWAYS applied, also when c >= n);
 *   Adam on g * coef.
 * A dropped step (a faulted fused launch, a data-parallel gradient carrying the NaN mark) adds nothing to the history and
 * leaves the outputs alone.  `grads` keeps d loss / d params, unclipped.
 * The history lives on the device twice: `log` in step order, and the same values sorted ascending in one of two ping-pong
 * buffers -- sorted[count & 1] is current, the update writes sorted[(count + 1) & 1].  All pointers are device pointers.
 * ------------------------------------------------------------------------------------------------------ */
typedef struct gatres_autoclip {
  double* log;                     /* [capacity] norms in step order                                                       */
  double* sorted[2];               /* [capacity] each                                                                      */
  uint64_t* ctl;                   /* uint64[8]: [0] = count (entries in the history; zero it to reset), [4] = overflow flag
                                    * (a step found count == capacity: it was skipped); the rest is internal             */
  double* partials;                /* [partials_cap] sum-of-squares partials of the update's norm launch                     */
  double* norm_out;                /* [1] n of the last step that was not dropped                                          */
  double* clip_out;                /* [1] c of that step                                                                   */
  double* coef_out;                /* [1] coef of that step                                                                */
  int64_t capacity;                /* entries log and sorted[] hold; the caller grows them before the count gets there      */
  int32_t partials_cap;            /* >= gatres_autoclip_partials(P)                                                       */
  int32_t reserved;
  double percentile;               /* 0 .. 100                                                                             */
} gatres_autoclip_t;

/* Entries `partials` needs for a parameter vector of `count` floats. */
int32_t gatres_autoclip_partials(int64_t count);

/* gatres_adam_step with AutoClip in front, on a caller's flat gradient: two launches (norm partials, clip + Adam + history). */
int gatres_autoclip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                              uint64_t* step_counter, int64_t count, double lr, double beta1, double beta2, double eps,
                              double weight_decay, float grad_scale, const gatres_autoclip_t* ac, void* stream);

/* --------------------------------------------------------------------------------------------------------
 * One reference training iteration (train.py:159-190) enqueued natively:
 *   PHASE_MASK     device mask sampler (utils/auxil.py:166-182) -- skipped when node_ptr == NULL (caller's mask)
 *   PHASE_FORWARD  x[mask] = 0 ; out = model(x) ; loss = criterion(out[mask], y[mask]) and d loss / d out (MSE unless
 *                  GATRES_FLAG_LOSS_MAE / GATRES_FLAG_LOSS_SCE)
 *   PHASE_BACKWARD grads = d loss / d params
 *   PHASE_ADAM     torch.optim.Adam(lr, weight_decay) update, step counter on the device
 * `phases` selects which of them a call enqueues, so a data-parallel caller can run its gradient all-reduce
 * between BACKWARD and ADAM.  Everything is stream-ordered and allocation-free (hipGraph capturable).
 * ------------------------------------------------------------------------------------------------------ */
#define GATRES_PHASE_MASK     1
#define GATRES_PHASE_FORWARD  2
#define GATRES_PHASE_BACKWARD 4
#define GATRES_PHASE_ADAM     8
#define GATRES_PHASE_ALL      15

typedef struct gatres_train_step {
  gatres_model_t model;
  const gatres_graph_t* graph;     /* HOST pointer to the plan struct (its members are device pointers) */
  float* params;                   /* [P] flat parameters (layout above)                 */
  float* grads;                    /* [P]                                                */
  float* exp_avg;                  /* [P] Adam first moment                              */
  float* exp_avg_sq;               /* [P] Adam second moment                             */
  uint64_t* step_counter;          /* device uint64[2]: {optimizer step, ticket}         */
  const float* x;                  /* [N] node inputs (z-normed pressures)               */
  const float* y;                  /* [N] targets (== x before masking, train.py:162-163)*/
  uint8_t* mask;                   /* [N] 1 = masked node                                */
  const int32_t* node_ptr;         /* [B+1] graph node offsets, or NULL                  */
  int32_t num_graphs;
  int32_t phases;
  double mask_rate;
  uint64_t seed;
  float* out;                      /* [N] predictions                                    */
  float* g_out;                    /* [N] d loss / d out                                 */
  float* loss;                     /* [1]                                                */
  float* saved;                    /* gatres_saved_floats()                              */
  float* scratch;                  /* gatres_scratch_floats()                            */
  double lr, beta1, beta2, eps, weight_decay;
  float grad_scale;                /* multiplies grads inside Adam (1/world_size)        */
  int32_t flags;                   /* GATRES_FLAG_PER_OP: force the per-op kernels       */
  const double* hparams;           /* device double[5] {lr, beta1, beta2, eps, weight_decay}, or NULL.  When set, the update
                                    * kernels read the hyper-parameters from it INSTEAD of the five host values above, so a
                                    * captured step follows a learning-rate schedule (train.py:349-350,510) without being
                                    * captured again                                                                     */
  int32_t block_lo, block_hi;      /* GATRES_FLAG_GRADS_ONLY: the blocks whose parameter gradients this call forms       */
  uint8_t* mask_next;              /* GATRES_FLAG_MASK_NEXT: [N] where the update launch leaves the NEXT step's mask (another
                                    * buffer than `mask`, which keeps the mask this step used); NULL: no sampling ahead     */
  const gatres_autoclip_t* autoclip; /* HOST pointer: PHASE_ADAM clips the gradient with AutoClip first (see gatres_autoclip_t);
                                    * NULL: no clipping, exactly the ABI-6 step                                            */
} gatres_train_step_t;
#define GATRES_FLAG_PER_OP 1
/* Fused path, PHASE_BACKWARD: stop after the backward chain; the caller forms the parameter gradients itself, range by
 * range, with gatres_fused_param_grads_finish (the data-parallel step: a bucket's all-reduce starts between two ranges). */
#define GATRES_FLAG_GRADS_DEFERRED 4
/* Fused path, PHASE_BACKWARD: ONLY the parameter gradients of blocks [block_lo, block_hi) from the kept tables of a
 * GRADS_DEFERRED backward (gatres_fused_param_grads_finish, no Adam; the launch that holds the last block also writes the
 * loss).  Needs gatres_fused_finish_folds(). */
#define GATRES_FLAG_GRADS_ONLY 8
/* Fused path, PHASE_ADAM in the same call as PHASE_BACKWARD, node_ptr and mask_next given: the update launch also samples
 * the mask of the NEXT step into `mask_next` (gatres_fused_finish_hp), so the next call -- with that buffer as its `mask` --
 * may leave PHASE_MASK out. */
#define GATRES_FLAG_MASK_NEXT 16
/* The transposed conv weights in `scratch` already match `params`: true right after a fused PHASE_ADAM step on the
 * same scratch (its Adam pass rewrites them) as long as nobody else has touched the parameters; skips the transposes. */
#define GATRES_FLAG_WT_VALID 2
/* The training criterion (gatres_masked_loss): GATRES_FLAG_LOSS_MAE -> nn.L1Loss, GATRES_FLAG_LOSS_SCE -> sce_loss; neither:
 * MSE.  Both: GATRES_E_BADARG.  Every path of the step honours it (the loss is formed in the forward phase). */
#define GATRES_FLAG_LOSS_MAE 32
#define GATRES_FLAG_LOSS_SCE 64

int gatres_train_step(const gatres_train_step_t* ts, void* stream);

/* --------------------------------------------------------------------------------------------------------
 * The epoch boundary of the reference's training loop (train.py:426-511) on the device: GATResTrainer.fit.
 * ------------------------------------------------------------------------------------------------------ */
typedef struct gatres_epoch_config {
  double min_delta;           /* EarlyStopping(mode="min", min_delta, patience): compared in fp32                        */
  double factor;              /* ReduceLROnPlateau(mode="min", patience=scheduler_patience): torch's defaults are        */
  double threshold;           /*   factor 0.1, threshold 1e-4 (relative), min_lr 0, eps 1e-8, cooldown 0 (fixed here)    */
  double min_lr;
  double eps;
  int32_t patience;           /* 0: early stopping never stops                                                            */
  int32_t scheduler_patience;
  int32_t use_scheduler;      /* 0: the learning rate is left alone                                                       */
  int32_t reserved;
} gatres_epoch_config_t;

/* The controller's persistent state: GATRES_EPOCH_STATE doubles.  Initial value: all 0 except BEST_LOSS = SCHED_BEST = +inf. */
#define GATRES_EPOCH_STATE 10
#define GATRES_EPOCH_S_EPOCH 0        /* epochs decided so far                                   */
#define GATRES_EPOCH_S_BEST_LOSS 1
#define GATRES_EPOCH_S_BEST_EPOCH 2
#define GATRES_EPOCH_S_ES_HAS_BEST 3  /* EarlyStopping.best is set                               */
#define GATRES_EPOCH_S_ES_BEST 4      /* an fp32 value                                           */
#define GATRES_EPOCH_S_ES_BAD 5
#define GATRES_EPOCH_S_SCHED_BEST 6
#define GATRES_EPOCH_S_SCHED_BAD 7
#define GATRES_EPOCH_S_IMPROVED 8     /* the last epoch improved best_loss: gatres_snapshot_if's flag */
#define GATRES_EPOCH_S_STOPPED 9
/* One history record per epoch: GATRES_EPOCH_RECORD doubles. */
#define GATRES_EPOCH_RECORD 16
#define GATRES_EPOCH_R_EPOCH 0
#define GATRES_EPOCH_R_TR_LOSS 1
#define GATRES_EPOCH_R_VAL_LOSS 2
#define GATRES_EPOCH_R_LR_USED 3      /* hp[0] during the epoch                                  */
#define GATRES_EPOCH_R_LR_AFTER 4     /* hp[0] after the scheduler's step                        */
#define GATRES_EPOCH_R_IMPROVED 5
#define GATRES_EPOCH_R_BEST_LOSS 6
#define GATRES_EPOCH_R_BEST_EPOCH 7
#define GATRES_EPOCH_R_ES_BAD 8
#define GATRES_EPOCH_R_STOP 9
#define GATRES_EPOCH_R_SCHED_BAD 10
#define GATRES_EPOCH_R_SCHED_BEST 11
#define GATRES_EPOCH_R_ES_BEST 12
#define GATRES_EPOCH_R_VAL_GRAPHS 13  /* [14..15] 0                                              */

/* The decision of one epoch as ONE single-wave launch, in the reference's order:
 *   1. tr_loss = train_sums[0] / train_sums[1] (the epoch's fp64 loss sum and graph count); val_loss = sum_b loss_b g_b / n,
 *      accumulated in fp64 batch by batch (product and sum each rounded), n = sum_b g_b, g_b = val_graphs[b], and
 *      loss_b = val_table[b][1] / val_table[b][0] (moment records of gatres_masked_metrics) or val_losses[b] (fp32, e.g.
 *      gatres_masked_loss) -- exactly one of the two is given.  num_batches == 0: val_sums = {sum_b loss_b g_b, n} instead
 *      (data parallel: the all-reduced sums of gatres_epoch_val_sums);
 *   2. improved = val_loss < best_loss (fp64, strict), best_epoch;
 *   3. EarlyStopping.step on the fp32 value of val_loss: the first epoch only stores it; a NaN stops; otherwise
 *      val < best - min_delta in fp32 resets the bad-epoch count, anything else counts; stop at count >= patience;
 *   4. unless stopped, ReduceLROnPlateau.step(val_loss) in fp64; a new learning rate is written to hp[0] (hp: the double[5] the
 *      update kernels read, gatres_train_step_t.hparams; hp[1..4] are not touched);
 *   5. history[epoch - 1] (if epoch <= history_capacity) and the state.
 * config_host is read by the call (HOST pointer); every other pointer is a device pointer. */
int gatres_epoch_control(const double* train_sums, const double* val_table, const float* val_losses,
                         const int32_t* val_graphs, int32_t num_batches, const double* val_sums,
                         const gatres_epoch_config_t* config_host, double* hp, double* state, double* history,
                         int32_t history_capacity, void* stream);

/* out[0] = sum_b loss_b g_b, out[1] = n, formed as gatres_epoch_control forms them (one rank's share under data parallelism). */
int gatres_epoch_val_sums(const double* val_table, const float* val_losses, const int32_t* val_graphs, int32_t num_batches,
                          double* out, void* stream);

/* The best checkpoint kept on the device: if flag[0] != 0 (flag == NULL: always) copy params, exp_avg, exp_avg_sq (count
 * floats each) and step_counter[0] to the dst_* buffers; otherwise nothing is written.  The flag is read by the kernel, so
 * the host enqueues the call unconditionally (flag = state + GATRES_EPOCH_S_IMPROVED).  Restoring is the same call with
 * sources and destinations exchanged and flag == NULL.  step_counter / dst_step_counter: both or neither. */
int gatres_snapshot_if(const double* flag, const float* params, const float* exp_avg, const float* exp_avg_sq,
                       const uint64_t* step_counter, float* dst_params, float* dst_exp_avg, float* dst_exp_avg_sq,
                       uint64_t* dst_step_counter, int64_t count, void* stream);

/* --------------------------------------------------------------------------------------------------------
 * Gradient flow and model update per epoch (train.py:476-504 with --log_gradient; k_grad_flow.hip).  New symbols only: the
 * ABI version stays (see GATRES_ABI_VERSION).
 * ------------------------------------------------------------------------------------------------------ */

/* get_gradient_norm(model, norm_type=2) (utils/auxil.py:295-313) on a flat gradient in the parameter layout above: the L2 norm
 * of every parameter tensor whose name contains "block" -- per block conv1.att_src, conv1.att_dst, conv1.bias,
 * conv1.lin.weight, conv2.att_src, conv2.att_dst, conv2.bias, conv2.lin.weight, the order of named_parameters(); lin0 / lin1
 * are left out -- and the norm of those norms.  out: device double[1 + gatres_grad_flow_count()]:
 *   out[1 + t] = sqrt(sum_i (double)g_i^2) * |scale| * c   over tensor t
 *   out[0]     = sqrt(sum_t sumsq_t) * |scale| * c
 * c = coef ? coef[0] : 1 (device double[1], read by the kernel).  `scale` is the factor the update applies to the gradient
 * (gatres_train_step_t.grad_scale), `coef` AutoClip's coefficient of the last update (gatres_autoclip_t.coef_out): the reference
 * reads .grad after clip_grad_norm_ scaled it in place, this engine keeps `grads` unclipped.  The tensor boundaries follow from
 * (num_blocks, nc).  One launch, one workgroup per tensor and one for the total; fp64 sums in a fixed order, no atomics: the
 * same bits on every run.  A NaN in a tensor gives NaN for that tensor and for out[0]; an all-zero tensor gives 0. */
int gatres_grad_flow(const gatres_model_t* m, const float* grads, double scale, const double* coef, double* out, void* stream);
int32_t gatres_grad_flow_count(int32_t num_blocks, int32_t nc);   /* 8 * num_blocks */

/* out[0] = (sum_i (double)fabsf(a_i - b_i)) / n: torch.abs(a - b).mean() with the difference and the absolute value in fp32, as
 * torch forms them, and the sum in fp64 in a fixed order (one workgroup). */
int gatres_mean_abs_diff(const float* a, const float* b, int64_t n, double* out, void* stream);

/* --------------------------------------------------------------------------------------------------------
 * Pressure estimation with a fixed sensor set (estimation.PressureEstimator; k_estimate.hip).  New symbols only: the ABI version
 * stays.
 * ------------------------------------------------------------------------------------------------------ */

/* One batch's input for a FIXED set of observed nodes, in one launch.  observed[num_observed] (device int32): node indices inside
 * a graph, distinct, each in [0, nodes_per_graph); 1 <= num_observed <= nodes_per_graph.  For g in [0, num_graphs):
 *   mask[g * N + v] = 1, x_dst[g * N + v] = 0.0f   at every node that is not observed,
 *   mask[g * N + v] = 0, x_dst[g * N + v] = value  at v = observed[k].
 * Every byte of mask and every float of x_dst in [0, num_graphs * N) is written exactly once: no memset beforehand.
 * layout GATRES_OBSERVED_FULL_ROWS: src is a snapshot matrix [src_rows][N], already scaled; graph g takes row
 *   rows ? rows[g] : first_row + g (rows: device int64), column observed[k], unchanged.
 * layout GATRES_OBSERVED_READINGS: src is [src_rows][num_observed] in physical units; graph g takes row first_row + g (rows must
 *   be NULL), column k for node observed[k], normalised as `normalise` says with o = (float)offset, f = (float)factor:
 *     GATRES_NORMALISE_NONE        value = r
 *     GATRES_NORMALISE_DIVIDE      value = fp32(fp32(r - o) / f)
 *     GATRES_NORMALISE_RECIPROCAL  value = fp32(fp32(r - o) * fp32(1.0f / f))   (torch's device kernel for tensor / host scalar)
 * A row outside [0, src_rows) named by rows[] is not read (its observed nodes get 0); without rows, first_row + num_graphs must
 * not pass src_rows. */
#define GATRES_OBSERVED_FULL_ROWS 0
#define GATRES_OBSERVED_READINGS  1
#define GATRES_NORMALISE_NONE       0
#define GATRES_NORMALISE_DIVIDE     1
#define GATRES_NORMALISE_RECIPROCAL 2
int gatres_stage_observed(const float* src, int32_t layout, int64_t src_rows, const int64_t* rows, int64_t first_row,
                          int32_t nodes_per_graph, int32_t num_graphs, const int32_t* observed, int32_t num_observed,
                          int32_t normalise, double offset, double factor, float* x_dst, uint8_t* mask, void* stream);

/* One batch's estimates into the result matrix dst[dst_rows][dst_stride] (physical units), in one launch:
 *   dst[(first_row + g) * dst_stride + v] = mask[g*N+v] ? D(out[g*N+v]) : (keep_observed ? D(x[g*N+v]) : D(out[g*N+v]))
 * with D(s) = fp32(fp32(s * (float)scale) + (float)offset), gatres_masked_metrics' rounding.  out, x, mask: the forward's
 * prediction, the staged input and the mask of gatres_stage_observed (x and mask may be NULL when keep_observed == 0).
 * dst_stride >= nodes_per_graph; first_row + num_graphs <= dst_rows; nothing outside the batch's rows and columns is written. */
int gatres_estimate_write(const float* out, const float* x, const uint8_t* mask, int32_t nodes_per_graph, int32_t num_graphs,
                          double scale, double offset, int32_t keep_observed, float* dst, int64_t dst_rows, int64_t dst_stride,
                          int64_t first_row, void* stream);

/* Per-node error moments of an estimate matrix est[S][N] (physical units) against the scaled truth[S][N], t = D(truth) as above,
 * e = fp32(p - t): table[N][GATRES_NODE_ERROR_RECORD] (device double), per node v over the snapshots s = 0 .. S - 1:
 *   [0] S   [1] sum e   [2] sum |e|   [3] sum e^2   [4] max |e|   [5] #{|t| > 0.01f}   [6] sum over those of |e| / |t|
 *   [7] 1.0 if v is in observed[num_observed], else 0.0
 * Observed nodes get their moments like any other.  One launch; the lanes of a wave take consecutive nodes, the waves of a
 * workgroup take the rows of a chunk of GATRES_NODE_ERROR_CHUNK snapshots in turn; fp64 sums in a fixed order (the waves'
 * partials are added in wave order through LDS), no atomics: the same bits on every run. */
#define GATRES_NODE_ERROR_RECORD 8
#define GATRES_NODE_ERROR_CHUNK 64
int gatres_node_error_moments(const float* est, const float* truth, int64_t num_snapshots, int32_t nodes_per_graph, double scale,
                              double offset, const int32_t* observed, int32_t num_observed, double* table, void* stream);

/* Calibrated per-node error bounds (symbols only: the ABI stays).  Split-conformal calibration: per node ONE order statistic
 * per level of |e| over the snapshots of a held-out store; a new snapshot exchangeable with those lies inside the bound with
 * probability >= level, per node.
 *
 * gatres_node_error_quantiles: est, truth, scale, offset, e = fp32(est - D(truth)) and D() as in gatres_node_error_moments.
 *   available  NULL: every entry (s, v) is COUNTED and observed / num_observed are not read.  Device uint8 [S][num_observed]:
 *              the entry is counted when it is hidden in the sense of gatres_node_error_moments_available, that is unless
 *              v == observed[k] and available[s * K + k] != 0.
 *   levels     HOST double[num_levels], each in the open interval (0, 1); read before the call returns.
 *   bounds     device float [num_levels][N];  counts: device double [N].
 * Per node v, A_v is the multiset of the 32-bit patterns of fabsf(e) over the counted entries, ordered as unsigned integers:
 * the IEEE order for finite values and +inf, a NaN above +inf, -0.0 and +0.0 one element.  n_v = |A_v|, counts[v] = n_v.  For
 * level q the rank is r = ceil((double)(n_v + 1) * levels[q]) (one fp64 product, one ceil; 1-based, r >= 1):
 *   r >  n_v   bounds[q * N + v] = +inf (too few samples; n_v == 0 included)
 *   r <= n_v   bounds[q * N + v] = the float whose bits are the r-th smallest element of A_v
 * exactly: a sort gives the same bits (estimation.node_error_bounds is that statement on the host), whatever the launch
 * geometry.  One launch: an MSB-first radix select, eight bits per pass, with histograms in LDS; every pass re-reads est and
 * truth.  No global atomics, no scratch in global memory, nothing written but bounds and counts.
 * GATRES_E_BADARG before any launch: a NULL est, truth, levels, bounds or counts; num_snapshots < 1 or above 2^31 - 1 (the
 * histograms count in 32 bits); nodes_per_graph < 1; num_levels outside [1, GATRES_NODE_QUANTILE_MAX_LEVELS]; a level that is
 * NaN or outside (0, 1); available != NULL with observed == NULL or num_observed outside [1, N]; bounds or counts overlapping
 * est, truth, available, observed or each other. */
#define GATRES_NODE_QUANTILE_MAX_LEVELS 8
int gatres_node_error_quantiles(const float* est, const float* truth, int64_t num_snapshots, int32_t nodes_per_graph,
                                double scale, double offset, const int32_t* observed, int32_t num_observed,
                                const uint8_t* available, const double* levels, int32_t num_levels, float* bounds,
                                double* counts, void* stream);

/* How many entries lie inside the bounds.  The inputs, e and the counted entries of gatres_node_error_quantiles; bounds: device
 * float [num_levels][N] (read).  table[N][1 + GATRES_NODE_QUANTILE_MAX_LEVELS] (device double), per node v over its counted
 * entries:
 *   [0] n_v   [1 + q] #{ fabsf(e) <= bounds[q * N + v] } by float comparison, q < num_levels   the other slots 0
 * A NaN error is never inside, a NaN bound covers nothing, a +inf bound covers every error that is no NaN.  The traversal of
 * gatres_node_error_moments; the counters are integers (exact as doubles), no atomics.
 * GATRES_E_BADARG before any launch: as gatres_node_error_quantiles, with bounds and table for levels, bounds and counts; table
 * overlapping est, truth, available, observed or bounds. */
int gatres_node_bound_coverage(const float* est, const float* truth, int64_t num_snapshots, int32_t nodes_per_graph,
                               double scale, double offset, const int32_t* observed, int32_t num_observed,
                               const uint8_t* available, const float* bounds, int32_t num_levels, double* table, void* stream);

/* Estimation when some sensor readings are missing (symbols only: the ABI stays).  A sensor without a reading in a snapshot is
 * one more hidden node of that snapshot: the model was trained with random masks.
 *
 * gatres_stage_observed with an availability: the arguments and checks of gatres_stage_observed, and
 *   available       device uint8 [src_rows][num_observed], non-zero: the reading is present.  It is indexed by the SOURCE row
 *                   r = rows ? rows[g] : first_row + g of graph g, like src.  NULL (every reading present) only with
 *                   nan_is_missing != 0; it must not overlap x_dst or mask.
 *   nan_is_missing  non-zero: in layout GATRES_OBSERVED_READINGS a raw reading that is a NaN is missing.  In layout
 *                   GATRES_OBSERVED_FULL_ROWS it has no effect: available alone decides.
 * At v = observed[k] of graph g:
 *   present  (available == NULL || available[r * K + k] != 0) and not (nan_is_missing, readings layout, reading is NaN):
 *            mask = 0, x_dst = the value exactly as gatres_stage_observed forms it (same normalisation, same rounding);
 *   missing  mask = 1, x_dst = 0.0f; the reading is not used (and not loaded when available says so).
 * Every other node: mask = 1, x_dst = 0.0f.  Every byte of mask and every float of x_dst of the batch is written exactly once,
 * in one launch of the same grid: the kernel of gatres_stage_observed compiled with the availability as a compile-time fact.  A
 * row outside [0, src_rows) named by rows[] is read in neither array (its observed nodes get mask = 0, x_dst = 0, as there).
 * GATRES_E_BADARG before any launch: whatever gatres_stage_observed refuses, available == NULL with nan_is_missing == 0, and an
 * available that overlaps x_dst or mask. */
int gatres_stage_observed_available(const float* src, int32_t layout, int64_t src_rows, const int64_t* rows, int64_t first_row,
                                    int32_t nodes_per_graph, int32_t num_graphs, const int32_t* observed, int32_t num_observed,
                                    int32_t normalise, double offset, double factor, float* x_dst, uint8_t* mask,
                                    const uint8_t* available, int32_t nan_is_missing, void* stream);

/* gatres_node_error_moments over the HIDDEN entries only.  available: device uint8 [S][num_observed], required.  The entry
 * (s, v) is hidden unless v == observed[k] and available[s * K + k] != 0.  table[N][GATRES_NODE_ERROR_AVAIL_RECORD] (device
 * double), per node v over its hidden entries, with e, t and D() as in gatres_node_error_moments:
 *   [0] number of hidden entries   [1] sum e   [2] sum |e|   [3] sum e^2   [4] max |e|   [5] #{|t| > 0.01f}
 *   [6] sum over those of |e| / |t|   [7] number of snapshots in which v was observed ([0] + [7] == S)
 * The traversal and the order of the fp64 sums are those of gatres_node_error_moments and an entry that is not hidden adds
 * nothing: a node outside observed[] gets that kernel's record bit for bit, a sensor present in every snapshot [0] = 0,
 * [7] = S and zero sums.  Only the lanes of sensor nodes read available.  One launch, no atomics: the same bits on every run. */
#define GATRES_NODE_ERROR_AVAIL_RECORD 8
int gatres_node_error_moments_available(const float* est, const float* truth, int64_t num_snapshots, int32_t nodes_per_graph,
                                        double scale, double offset, const int32_t* observed, int32_t num_observed,
                                        const uint8_t* available, double* table, void* stream);

/* Estimates and their spread under sensor noise (symbols only: the ABI stays).  A Monte-Carlo ensemble of `members` noisy
 * realisations per snapshot is one long pass over (snapshot, member) PAIRS, snapshot-major: pair p is source row p / members
 * and member p % members.
 *
 * gatres_stage_observed_noisy: the kernel of gatres_stage_observed_available compiled with the noise as one more compile-time
 * fact.  The arguments, the layouts and the checks of gatres_stage_observed_available, without rows, and
 *   first_pair   graph g of the launch is pair p = first_pair + g: it reads source row p / members (of src and of available)
 *                and is member member0 + p % members.  0 <= first_pair, first_pair + num_graphs <= src_rows * members.
 *   members      >= 1;  member0 >= 0 (a single realisation: members = 1, member0 = its member)
 *   sigma        device float[num_observed], >= 0, in the units of src (layout GATRES_OBSERVED_FULL_ROWS: normalised units)
 *   seed         any 64-bit value
 *   available    may be NULL with nan_is_missing == 0 here: every reading is present.
 * At a PRESENT sensor k with the raw value r (src[row * K + k] in the readings layout, src[row * N + observed[k]] in full rows):
 *   x_dst = normalise(fp32(r + fp32(sigma[k] * z)))   (normalise: as gatres_stage_observed, the identity for full rows)
 * A missing reading draws nothing and is staged as gatres_stage_observed_available stages it.  z is a pure function of
 * (seed, member, source row, k) -- not of the batch, the graph's position in it, the availability or the launch geometry --
 * with mix64(z) = { z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31; } and
 * all integer arithmetic modulo 2^64:
 *   stream = mix64(seed + 0x9E3779B97F4A7C15 * (member + 1))
 *   h      = mix64(stream + 0xBF58476D1CE4E5B9 * (row * K + k + 1))
 *   u1     = ((h >> 40) + 1) * 2^-24   in (0, 1],   u2 = ((h >> 8) & 0xFFFFFF) * 2^-24   in [0, 1)   (both exact in fp32)
 *   z      = sqrtf(-2 * logf(u1)) * cosf(6.283185307179586f * u2)      (|z| <= sqrt(48 ln 2) = 5.77)
 * estimation.reading_noise restates it on the host.  GATRES_E_BADARG before any launch: whatever
 * gatres_stage_observed_available refuses (but for the NULL available), a pair range outside [0, src_rows * members),
 * members < 1, member0 < 0, sigma == NULL or overlapping x_dst or mask. */
int gatres_stage_observed_noisy(const float* src, int32_t layout, int64_t src_rows, int64_t first_pair, int32_t members,
                                int64_t member0, int32_t nodes_per_graph, int32_t num_graphs, const int32_t* observed,
                                int32_t num_observed, int32_t normalise, double offset, double factor, float* x_dst, uint8_t* mask,
                                const uint8_t* available, int32_t nan_is_missing, const float* sigma, uint64_t seed, void* stream);

/* Mean and sample standard deviation over the members of each snapshot.  members_mat[num_snapshots * members][stride] is what
 * gatres_estimate_write produced with the pair index as the row; mean and std_dev are [out_rows][out_stride] and get the rows
 * first_row + s, columns [0, nodes_per_graph); nothing else is written.  Per (s, v), in fp64, in member order m = 0 .. M - 1,
 * without contraction and without atomics (the same bits on every run, whatever the launch geometry):
 *   mean64 = (sum_m (double)x_m) / M        var = (sum_m (x_m - mean64)^2) / (M - 1)
 *   mean   = (float)mean64                  std_dev = (float)sqrt(var), 0 for M == 1
 * One launch; the lanes of a wave take consecutive v, in 16-byte accesses where nodes_per_graph, both strides and the three
 * pointers allow it.  GATRES_E_BADARG before any launch: members < 1, a stride below nodes_per_graph, rows outside
 * [0, out_rows), and source, mean rows and std_dev rows that overlap one another. */
int gatres_ensemble_reduce(const float* members_mat, int64_t num_snapshots, int32_t members, int32_t nodes_per_graph,
                           int64_t stride, float* mean, float* std_dev, int64_t out_rows, int64_t out_stride, int64_t first_row,
                           void* stream);

/* Per-node moments of a matrix of standard deviations std_dev[S][N] (gatres_ensemble_reduce's, contiguous):
 * table[N][GATRES_NODE_SPREAD_RECORD] (device double), per node v over the snapshots s = 0 .. S - 1:
 *   [0] S   [1] sum (double)sd * (double)sd   [2] max sd   [3] sum (double)sd
 * The geometry and the fixed summation order of gatres_node_error_moments (chunks of GATRES_NODE_ERROR_CHUNK rows). */
#define GATRES_NODE_SPREAD_RECORD 4
int gatres_node_spread_moments(const float* std_dev, int64_t num_snapshots, int32_t nodes_per_graph, double* table, void* stream);

/* Scoring sensor layouts (symbols only: the ABI stays).  A sensor layout is a subset of the estimator's observed[] (the candidate
 * sensors): layouts[L][num_observed] (device uint8), non-zero: sensor k is installed in that layout.  Scoring L layouts over S
 * snapshots is one long pass over (snapshot, layout) PAIRS, snapshot-major: pair p is source row p / L and layout p % L.  Per
 * batch of pairs: gatres_stage_observed_layouts, the forward, gatres_layout_pair_errors (one small record per pair, read from the
 * forward's buffers: no estimate matrix); per chunk of snapshots one gatres_layout_error_reduce.
 *
 * gatres_stage_observed_layouts: the kernel of gatres_stage_observed_available compiled with the layout as one more compile-time
 * fact.  The arguments, the source layouts and the checks of gatres_stage_observed_available, without rows, and
 *   first_pair   graph g of the launch is pair p = first_pair + g: it reads source row p / num_layouts (of src and of available)
 *                under layout p % num_layouts.  0 <= first_pair, first_pair + num_graphs <= src_rows * num_layouts.
 *   num_layouts  >= 1
 *   layouts      device uint8 [num_layouts][num_observed], required; it must not overlap x_dst or mask
 *   available    [src_rows][num_observed]; may be NULL with nan_is_missing == 0 here: every reading is there.
 * At v = observed[k] of graph g the reading is PRESENT when layouts[(p % L) * K + k] != 0 and (available == NULL or
 * available[(p / L) * K + k] != 0) and it is no NaN under nan_is_missing in the readings layout: mask = 0, x_dst = the value
 * exactly as gatres_stage_observed forms it (same normalisation, same rounding).  Everything else -- a sensor the layout leaves
 * out, a missing reading, a node without a sensor -- gets x_dst = 0.0f, mask = 1; a reading that is not present is not loaded
 * where layouts or available says so.  Every byte of mask and every float of x_dst of the batch is written exactly once.
 * GATRES_E_BADARG before any launch: whatever gatres_stage_observed_available refuses (but for the NULL available),
 * layouts == NULL or overlapping x_dst or mask, a pair range outside [0, src_rows * num_layouts), num_layouts < 1. */
int gatres_stage_observed_layouts(const float* src, int32_t layout, int64_t src_rows, int64_t first_pair, int32_t num_layouts,
                                  int32_t nodes_per_graph, int32_t num_graphs, const int32_t* observed, int32_t num_observed,
                                  int32_t normalise, double offset, double factor, float* x_dst, uint8_t* mask,
                                  const uint8_t* available, int32_t nan_is_missing, const uint8_t* layouts, void* stream);

/* One batch's error, one record per graph.  out, mask: the forward's prediction and the staged mask of the batch,
 * [num_graphs * N]; truth: the store's scaled matrix [truth_rows][N]; graph g is pair p = first_pair + g and is compared with
 * truth row s = p / num_layouts.  The nodes counted are those with mask[g*N+v] != 0 && (score == NULL || score[v] != 0) (score:
 * device uint8 [N]): the hidden nodes of the pair, or those of them that a caller's pool names.  With D() as in
 * gatres_estimate_write and e = fp32(D(out[g*N+v]) - D(truth[s*N+v])), the e of gatres_node_error_moments at a hidden node,
 * rec[rec_first + g][GATRES_LAYOUT_PAIR_RECORD] (device double) gets
 *   [0] nodes counted   [1] sum (double)|e|   [2] sum (double)e * (double)e   [3] max |e|
 * and four zeros when nothing is counted; nothing but the batch's num_graphs records is written.  One wave per graph; a lane
 * takes chunks of four consecutive nodes (16-byte loads of out and truth, 32-bit loads of mask and score, where g * N, s * N and
 * the pointers allow), the chunks of a wave are consecutive.  fp64 sums in an order that is a function of N alone (a lane's
 * terms in node order, the lanes by a fixed butterfly), no atomics: the same bits on every run and in every batch composition.
 * GATRES_E_BADARG before any launch: a NULL out, mask, truth or rec, num_layouts < 1, a pair range outside
 * [0, truth_rows * num_layouts), records outside [0, rec_rows), rec[rec_rows] overlapping out, mask, truth or score. */
#define GATRES_LAYOUT_PAIR_RECORD 4
int gatres_layout_pair_errors(const float* out, const uint8_t* mask, const float* truth, int64_t truth_rows,
                              int32_t nodes_per_graph, int32_t num_graphs, int64_t first_pair, int32_t num_layouts, double scale,
                              double offset, const uint8_t* score, double* rec, int64_t rec_rows, int64_t rec_first, void* stream);

/* The records of num_snapshots * num_layouts pairs, snapshot-major (rec[(s * L + l)][GATRES_LAYOUT_PAIR_RECORD]), folded into
 * table[L][GATRES_LAYOUT_ERROR_RECORD] (device double).  Per layout l, strictly in the order s = 0 .. num_snapshots - 1:
 *   [0] += count   [1] += sum |e|   [2] += sum e^2   [3] = fmax([3], max |e|)
 * from zero when accumulate == 0, from the table's current record otherwise: a pass cut into chunks of snapshots (the first
 * launch with accumulate == 0, the others with 1) leaves the bits of one launch over all of them.  One lane per layout,
 * consecutive lanes read consecutive records; no atomics.  GATRES_E_BADARG before any launch: a NULL pointer, num_snapshots < 1,
 * num_layouts < 1, rec overlapping table. */
#define GATRES_LAYOUT_ERROR_RECORD 4
int gatres_layout_error_reduce(const double* rec, int64_t num_snapshots, int32_t num_layouts, double* table, int32_t accumulate,
                               void* stream);

/* Sensitivity of the estimates to each sensor reading (symbols only: the ABI stays; k_sensitivity.hip).  The Jacobian
 * J[j][k] = d estimate_j / d reading_k in reverse mode: one graph of a batch carries ONE target junction j, its seed is
 * g_out = e_j, and g_x = d out_j / d x of gatres_model_backward at the sensor nodes is row j of J.  Computing T rows for each of
 * S snapshots is one long pass over (snapshot, target) PAIRS, snapshot-major: pair p is source row p / T and target p % T.  Per
 * batch of pairs: gatres_stage_observed_targets, gatres_model_forward with a saved buffer, gatres_model_backward with g_x,
 * gatres_sensitivity_gather.
 *
 * gatres_stage_observed_targets: the kernel of gatres_stage_observed_available compiled with the targets as one more compile-time
 * fact.  The arguments, the source layouts and the checks of gatres_stage_observed_layouts, without layouts, and
 *   first_pair   graph g of the launch is pair p = first_pair + g: it reads source row p / num_targets (of src and of available)
 *                and is staged exactly as gatres_stage_observed_available stages that row (with available == NULL and
 *                nan_is_missing == 0, legal here: as gatres_stage_observed stages it).
 *                0 <= first_pair, first_pair + num_graphs <= src_rows * num_targets.
 *   num_targets  T >= 1
 *   targets      device int32 [T], each in [0, N): target t is node targets[t].  NULL: target t is node t, which needs T <= N.
 *                A value outside [0, N) seeds nothing (its graph's g_out is all zero).
 *   g_out        device float [num_graphs * N]:  g_out[g * N + v] = (v == target(p % T)) ? 1.0f : 0.0f
 * Every float of x_dst and g_out and every byte of mask of the batch is written exactly once, from the same chunks of the same
 * grid: no memset beforehand.  g_out is stored 16 bytes at a time where x_dst is and g_out is aligned so, element by element
 * otherwise.  GATRES_E_BADARG before any launch: whatever gatres_stage_observed_layouts refuses of the arguments they share, a
 * NULL g_out, a g_out that overlaps x_dst, mask, src or targets, targets overlapping x_dst or mask, num_targets < 1, a NULL
 * targets with num_targets > N, a pair range outside [0, src_rows * num_targets). */
int gatres_stage_observed_targets(const float* src, int32_t layout, int64_t src_rows, int64_t first_pair, int32_t num_targets,
                                  const int32_t* targets, int32_t nodes_per_graph, int32_t num_graphs, const int32_t* observed,
                                  int32_t num_observed, int32_t normalise, double offset, double factor, float* x_dst,
                                  uint8_t* mask, float* g_out, const uint8_t* available, int32_t nan_is_missing, void* stream);

/* One batch's rows of J[J_rows][J_stride] (device float), one launch.  g_x, mask: [num_graphs * N], the backward's input
 * gradient and the staged mask of the batch; observed[num_observed] as in gatres_stage_observed.  For g in [0, num_graphs),
 * k in [0, K):
 *   J[(first_row + g) * J_stride + k] = mask[g*N + observed[k]] ? 0.0f : fp32(g_x[g*N + observed[k]] * (float)unit)
 * one fp32 product, rounded once.  The mask decides: the fused kernels write g_x at every node, so the entry of a sensor that is
 * missing or hidden means nothing and reads as exactly 0, whatever it holds (a NaN included).  unit = scale / factor of the
 * descale and of the normalisation turns d out / d x into physical units per physical unit.
 *   fault   device float, may be NULL.  When *fault is a NaN, every J of the batch is a NaN.  The caller passes the last float
 *           of the backward's parameter gradient (lin1.bias), which a split launch whose partner never arrived turns into NaN
 *           (see the fused per-snapshot path above).
 * Nothing outside the batch's rows and the K columns is written.  GATRES_E_BADARG before any launch: a NULL g_x, mask, observed
 * or J, num_observed outside [1, N], J_stride < num_observed, rows outside [0, J_rows), the batch's rows of J overlapping g_x,
 * mask, observed or fault. */
int gatres_sensitivity_gather(const float* g_x, const uint8_t* mask, const float* fault, int32_t nodes_per_graph,
                              int32_t num_graphs, const int32_t* observed, int32_t num_observed, double unit, float* J,
                              int64_t J_rows, int64_t J_stride, int64_t first_row, void* stream);

/* The rows of num_snapshots * num_targets pairs, pair-major (J[(s * T + t)][J_stride]), folded into
 * table[T][K][GATRES_SENSITIVITY_RECORD] (device double).  Per (t, k), strictly in the order s = 0 .. num_snapshots - 1, with
 * j = (double)J[(s * T + t) * J_stride + k]:
 *   [0] += 1 where j != 0 (a NaN counts)   [1] += j   [2] += |j|   [3] += j * j   [4] = fmax([4], |j|)
 * from zero when accumulate == 0, from the table's current record otherwise: a pass cut into chunks of snapshots (the first
 * launch with accumulate == 0, the others with 1) leaves the bits of one launch over all of them.  fp64, no contraction, no
 * atomics; one lane per (t, k), consecutive lanes read consecutive floats.  GATRES_E_BADARG before any launch: a NULL pointer,
 * num_snapshots < 1, num_targets < 1, num_observed < 1, J_stride < num_observed, J overlapping table. */
#define GATRES_SENSITIVITY_RECORD 5
int gatres_sensitivity_fold(const float* J, int64_t num_snapshots, int32_t num_targets, int32_t num_observed, int64_t J_stride,
                            double* table, int32_t accumulate, void* stream);

/* The first-order spread of every row of J[rows][J_stride] under independent reading errors of standard deviation
 * sigma[num_observed] (device float, in the units of the readings J was formed for):
 *   out[r] = (float)sqrt(sum_k ((double)J[r][k] * (double)sigma[k])^2)
 * summed in the order k = 0 .. K - 1, in fp64, every operation rounded once (the product of two floats is exact in fp64), without
 * contraction and without atomics, as gatres_ensemble_reduce sums: the same bits on every run.  GATRES_E_BADARG before any
 * launch: a NULL pointer, rows < 1, num_observed < 1, J_stride < num_observed, J, sigma and out overlapping one another. */
int gatres_sensitivity_spread(const float* J, int64_t rows, int32_t num_observed, int64_t J_stride, const float* sigma, float* out,
                              void* stream);

/* Screening of sensor readings (symbols only: the ABI stays; k_screen.hip).  A reading that is present and wrong -- stuck,
 * drifting, off by a constant -- shows in its LEAVE-ONE-OUT residual: the reading against the model's prediction at its node
 * with that one sensor hidden.  "Every sensor but k" is a layout: the S * K (snapshot, left-out sensor) PAIRS, snapshot-major,
 * are one long pass of gatres_stage_observed_layouts with layouts[K][K] = all ones, zero diagonal (pair p is source row p / K
 * under layout p % K), the forward and gatres_loo_residuals per batch; gatres_screen_reject then decides, per snapshot.
 *
 * gatres_loo_residuals: one batch of pairs.  out, mask: [num_graphs * N], the forward's prediction and the staged mask of the
 * batch; observed[K] as in gatres_stage_observed; src, layout, src_rows: the reading source of the staging launch, in either
 * layout; scale, offset: those of gatres_estimate_write, D() its descale (two roundings, no contraction).  Graph g is pair
 * p = first_pair + g: snapshot s = p / K, sensor k = p % K, node v = observed[k], and
 *   r = src[s * K + k]  (GATRES_OBSERVED_READINGS, physical units)   or   r = D(src[s * N + v])  (GATRES_OBSERVED_FULL_ROWS)
 *   pred[s * K + k]  = D(out[g * N + v])
 *   resid[s * K + k] = fp32(r - pred[s * K + k])
 * pred and resid: device float [src_rows][K].  The residual is the quiet NaN 0x7fc00000 (and pred is still written) when
 *   the reading is not there: available != NULL and available[s * K + k] == 0 (device uint8 [src_rows][K]; the reading is then
 *     not loaded), or nan_is_missing != 0 and r is a NaN;
 *   mask[g * N + v] == 0: the pair was not staged with its sensor hidden and the number would be the sensor looking at itself
 *     (gatres_sensitivity_gather guards its mask in the same way).
 * A NaN reading without nan_is_missing gives the NaN of the subtraction.  An observed[k] outside [0, N) reads nothing: pred and
 * resid are that quiet NaN.  Nothing but the batch's num_graphs entries of pred and of resid is written.  One graph per thread
 * and trip, a capped grid that strides over the graphs.
 * GATRES_E_BADARG before any launch: a NULL out, mask, src, observed, pred or resid; a layout that is neither of the two;
 * nodes_per_graph < 1, num_graphs < 1, num_observed outside [1, N]; src_rows < 1; a pair range outside [0, src_rows * K); the
 * batch's entries of pred or resid overlapping each other, out, mask, src, observed or available. */
int gatres_loo_residuals(const float* out, const uint8_t* mask, const float* src, int32_t layout, int64_t src_rows,
                         int64_t first_pair, int32_t nodes_per_graph, int32_t num_graphs, const int32_t* observed,
                         int32_t num_observed, double scale, double offset, const uint8_t* available, int32_t nan_is_missing,
                         float* pred, float* resid, void* stream);

/* One rejection round for num_snapshots snapshots, one launch.  resid[S][K] (device float); bound[K] and inv_bound[K] (device
 * float; the caller forms inv_bound = 1.0f / bound on the host, so no device division enters this statement); available[S][K]
 * (device uint8), UPDATED IN PLACE; rejected[S][max_rounds] (device int32), of which only column `round` is written; flagged
 * [S][K] (device uint8), may be NULL.  Sensor k of snapshot s is a CANDIDATE when
 *   available[s * K + k] != 0  and  resid[s * K + k] is no NaN  and  fabsf(resid[s * K + k]) > bound[k]   (float comparison)
 * so a NaN or +inf bound never yields a candidate.  flagged, when given, is the candidate indicator (1 / 0), written for every
 * (s, k).  Among the candidates of a snapshot the one with the largest score = fp32(fabsf(resid) * inv_bound[k]) is chosen, ties
 * going to the smallest k: the total order (score descending, k ascending), the scores ordered by IEEE value with -0 below +0
 * and a NaN score (possible only with an inv_bound that is not 1 / bound) below every other.  With n_s the number of non-zero
 * entries of row s of available:
 *   a candidate k* exists and n_s - 1 >= min_sensors:   available[s * K + k*] = 0,  rejected[s * max_rounds + round] = k*
 *   otherwise:                                           rejected[s * max_rounds + round] = -1,  available untouched
 * One wave per snapshot, the lanes stride over k; a lane's best and the butterfly over the lanes use that total order, so the
 * result is a function of the inputs alone, whatever the geometry.  The snapshots beyond the (capped) grid are taken by a loop.
 * GATRES_E_BADARG before any launch: a NULL resid, bound, inv_bound, available or rejected; num_snapshots < 1, num_observed < 1,
 * min_sensors < 1, max_rounds < 1, round outside [0, max_rounds); available, rejected or flagged overlapping resid, bound,
 * inv_bound or one another. */
int gatres_screen_reject(const float* resid, const float* bound, const float* inv_bound, uint8_t* available,
                         int64_t num_snapshots, int32_t num_observed, int32_t min_sensors, int32_t round, int32_t max_rounds,
                         int32_t* rejected, uint8_t* flagged, void* stream);

/* Drift monitoring of sensor readings (symbols only: the ABI stays; k_monitor.hip).  A sensor that drifts by a fraction of its
 * screening bound per step never exceeds a per-snapshot bound; a two-sided CUSUM per sensor along time sees it.  resid[S][K] is
 * the matrix gatres_loo_residuals writes, read as E = S / T independent SERIES of T = series_length consecutive rows (series e:
 * rows [eT, (e + 1)T)); first_index = t0 is the global time index of row 0 of every series, so that two calls on consecutive
 * chunks, the second with the first's state_out and t0 advanced, give what one call gives.
 *
 * gatres_cusum_scan.  mu[K], inv_sigma[K]: device float; available[S][K]: device uint8 or NULL; kappa_q, h_q: the allowance and
 * the threshold in units of 2^-16 sigma, llrint(kappa * 65536.0) formed by the caller.  All state is int64 in those units.
 * Entry (t, k) is COUNTED when available is NULL or non-zero there, resid is no NaN and
 *   z = fp32(fp32(resid - mu[k]) * inv_sigma[k])          (two roundings, no contraction)
 * is no NaN.  z is clamped to +-32768.0f, q = llrintf(z * 65536.0f), a+ = q - kappa_q, a- = -q - kappa_q.  The state per
 * (e, k) is int64[4] = {P, M, zP, zM}: from state_in (device [E][K][4]; P and M clamped into [0, 2^61] on entry) or, with
 * state_in == NULL, {0, 0, t0, t0}.  At a counted step with global index tau = t0 + t
 *   P = max(0, P + a+), and zP = tau + 1 if P == 0;     M = max(0, M + a-), and zM = tau + 1 if M == 0
 * and at any other step nothing changes.  The first counted step at which P > h_q or M > h_q (strictly) is the ALARM; if both
 * hold there the larger statistic wins, a tie going to +.  records[E][K][GATRES_CUSUM_RECORD] (device int64):
 *   [0] the alarm's tau, or -1   [1] side +1 / -1, or 0   [2] onset: zP or zM of that side after that step, the first snapshot
 *   of the excursion that alarmed   [3] n: the counted entries of this call with tau in [max(onset, t0), alarm]
 *   [4] the sum of q over those entries   [5] the alarming statistic                  ([1] .. [5] are 0 without an alarm)
 * The scan goes on after the alarm without a reset; state_out (device [E][K][4]; may be NULL, may equal state_in) is the state
 * after the last row.  stat_pos, stat_neg (device float [S][K], both or neither NULL) receive __ll2float_rn(P) * 2^-16f and the
 * same of M at every row, counted or not.
 * One workgroup per (series, sensor) on a capped grid that strides over the pairs; every thread owns a contiguous slice of the
 * T rows and folds it into the summary (A, C) of the map g -> max(C, g + A) per side, (A1, C1) o (A2, C2) = (A1 + A2,
 * max(C2, C1 + A2)) with the identity C = -2^62; an exclusive scan of the summaries (wave shuffles, LDS across waves) gives every
 * slice its carry-in, a second sweep walks the slice with the true values, an exclusive max-scan of the slices' last zeros and
 * a min-reduce of their first alarms give the record, a third sweep sums [3] and [4].  Integer addition and max are
 * associative: the bits of the sequential loop (monitoring.cusum_scan_ref), whatever the geometry.  No atomics.
 * GATRES_E_BADARG before any launch: a NULL resid, mu, inv_sigma or records; num_snapshots, num_observed or series_length < 1;
 * num_snapshots no multiple of series_length; series_length >= 2^30 (the bound that keeps every sum below 2^63);
 * first_index < 0 or above 2^61 - 1, a num_snapshots whose byte counts do not fit; kappa_q or h_q outside [0, 2^31]; one of stat_pos / stat_neg NULL and the other not; state_out, records,
 * stat_pos or stat_neg overlapping resid, mu, inv_sigma, available, state_in or one another (state_out == state_in excepted). */
#define GATRES_CUSUM_STATE 4
#define GATRES_CUSUM_RECORD 6
int gatres_cusum_scan(const float* resid, const float* mu, const float* inv_sigma, const uint8_t* available,
                      int64_t num_snapshots, int32_t num_observed, int64_t series_length, int64_t first_index, int64_t kappa_q,
                      int64_t h_q, const int64_t* state_in, int64_t* state_out, int64_t* records, float* stat_pos,
                      float* stat_neg, void* stream);

/* One latching round, one workgroup per series.  records[E][K][GATRES_CUSUM_RECORD] as gatres_cusum_scan writes them;
 * available[S][K] (device uint8), UPDATED IN PLACE; latched[E][max_rounds] (device int32), of which column `round` is written
 * and the columns before it are read; latched_rec[E][max_rounds][GATRES_CUSUM_RECORD] (device int64), of which row `round` is
 * written.  Sensor k is a CANDIDATE of series e when records[e][k][0] >= 0 and k is not in latched[e][0 .. round).  The
 * candidate with the smallest alarm index is chosen, ties going to the larger records[..][5], then to the smaller k: one total
 * order, used by a lane's own best and by the butterfly over the lanes.  If a candidate k* exists and
 * K - #{latched[e][r] >= 0, r < round} - 1 >= min_sensors:
 *   latched[e][round] = k*, latched_rec[e][round] = its record, and available[row][k*] = 0 for every row of the series with
 *   tau >= max(onset, t0) (since == 0) or tau >= alarm (since == 1);
 * otherwise latched[e][round] = -1, latched_rec[e][round] is six zeros and available is untouched.
 * GATRES_E_BADARG before any launch: a NULL pointer; num_snapshots, num_observed or series_length < 1; num_snapshots no multiple
 * of series_length; series_length >= 2^30; first_index < 0 or above 2^61 - 1; since other than 0 or 1; min_sensors < 1; max_rounds < 1; round
 * outside [0, max_rounds); available, latched or latched_rec overlapping records or one another. */
int gatres_monitor_latch(const int64_t* records, uint8_t* available, int64_t num_snapshots, int32_t num_observed,
                         int64_t series_length, int64_t first_index, int32_t since, int32_t min_sensors, int32_t round,
                         int32_t max_rounds, int32_t* latched, int64_t* latched_rec, void* stream);

/* Hydraulically consistent snapshots (symbols only: the ABI stays; k_hydraulics.hip, hydraulics.py).  THE MODEL, stated once:
 * a network of N nodes and P pipes; a node is a JUNCTION or a FIXED-HEAD node (a reservoir, or a tank held at a level).  The
 * analysis is demand-driven and steady, with Hazen-Williams in SI units.  Pipe p runs from node a_p to node b_p, carries the flow
 * q_p (m3/s, positive from a to b) and loses the head
 *   H_a - H_b = h_p(q_p),   h_p(q) = r_p |q|^0.852 q,   r_p = 10.667 L_p / (C_p^1.852 D_p^4.871)
 * (L, D in metres, C the Hazen-Williams roughness coefficient); at every junction, inflow - outflow = demand.  THE LAW AT LOW
 * FLOW (EPANET's rule, a part of the law and not of the solver), pipe_headloss(q, r) -> (h, g), every operation rounded to fp64:
 *   a = pow(|q|, 0.852);  ra = r * a;  g = 1.852 * ra;  h = ra * q;   where g < 1e-7:  g = 1e-7, h = 1e-7 * q.
 * THE SOLVER is Newton's method in the global-gradient form of Todini & Pilati, as in EPANET.  Flows start at
 * q_p = 0.3048 m/s * pi D_p^2 / 4 (1 ft/s).  One iteration: (h_p, g_p) = pipe_headloss(q_p, r_p), y_p = h_p / g_p; the symmetric
 * positive definite system A H = F over the junctions, with, for every pipe p at junction i and its other end j,
 *   A_ii += 1 / g_p;   A_ij -= 1 / g_p (j a junction)  or  F_i += H_j / g_p (j fixed);
 *   F_i = -demand_i + sum over pipes INTO i of (q_p - y_p) - sum over pipes OUT OF i of (q_p - y_p) + the fixed-head terms;
 * fixed nodes are identity rows (A_ff = 1, F_f = H_f); then dq_p = y_p - (H_a - H_b) / g_p and q_p <- q_p - dq_p.  The iteration
 * stops as CONVERGED once sum_p |dq_p| <= accuracy * sum_p |q_p| (the new flows), and otherwise after max_iter iterations.
 * WHAT DOES NOT HOLD: a flow that should be zero does not come to rest on the linear branch.  A head of 100 m resolves 1.4e-14 m
 * in fp64 and the linear branch turns a head difference into a flow with 1 / g = 1e7, so one ulp between neighbours is 1e-7 m3/s,
 * off the linear branch again.  Such flows jitter at 1e-7 .. 1e-6 m3/s between iterations and add that to sum |dq|: a scenario
 * of zero demand never meets the stop rule (heads right to 1e-7 m, converged 0), and one with many idle pipes may not either.
 *
 * gatres_hydraulic_draw: random scenarios.  d_lo, d_hi: device double[N]; c_lo, c_hi: device double[P]; it writes
 * demand[S][N] and roughness[S][P] (device double).  With all integer arithmetic modulo 2^64 and mix64 as stated at
 * gatres_stage_observed_noisy, scenario s of the call being the GLOBAL scenario g = first_scenario + s:
 *   stream = mix64(seed + 0x9E3779B97F4A7C15 * (g + 1))
 *   h      = mix64(stream + 0xBF58476D1CE4E5B9 * (cell + 1))      cell = i for demand[s][i],  N + p for roughness[s][p]
 *   u      = (h >> 11) * 2^-53                                    in [0, 1), exact in fp64
 *   value  = lo + (hi - lo) * u                                   the subtraction, the product and the sum rounded separately
 * so a value is a pure function of (seed, g, cell): chunks of scenarios give the bits of one call, and hydraulics.hydraulic_draws
 * gives them in numpy.  Fixed-head nodes are given d_lo = d_hi = 0 by the caller.  GATRES_E_BADARG before any launch: a NULL
 * pointer; num_scenarios, num_nodes or num_pipes < 1; first_scenario < 0 or first_scenario + num_scenarios above 2^62; demand
 * or roughness overlapping an input or one another.
 *
 * gatres_hydraulic_solve: one workgroup per scenario on a grid capped at GATRES_HYD_GRID_CAP; the scenarios beyond it are taken by
 * a loop.  STATIC inputs (device): pipe_a, pipe_b int32[P]; coef double[P] = 10.667 L / D^4.871 (so r = coef / pow(C, 1.852));
 * q_start double[P]; fixed uint8[N]; elevation double[N]; order int32[N] (solver row -> node) and position int32[N] (node ->
 * solver row), a permutation chosen by the caller for a narrow band; half_bandwidth W: |position[a] - position[b]| <= W for every
 * pipe between two junctions.  PER-SCENARIO inputs (device): demand double[S][N] (ignored at fixed nodes), roughness double[S][P],
 * fixed_head double, row s at fixed_head + s * fixed_head_stride, fixed_head_stride 0 (one row for all) or N (read at fixed
 * nodes only).  The lower band of A ((W + 1) doubles per row), the vectors and the pipe state live in LDS in fp64; the whole
 * Newton loop runs inside the kernel: assembly row by row over the pipes in pipe order, a banded LDL^T without pivoting, column
 * by column, with the forward substitution in the same sweep, the backward substitution column by column, and the two sums of the
 * stop rule added up in pipe order by one thread each.  Every order is fixed: a scenario's bits depend neither on S, nor on its
 * position, nor on the launch.  A shape whose LDS need
 *   8 * (N * (W + 1) + 2 N + 4 P) + 4 * (2 P + N) + 64 bytes
 * exceeds GATRES_HYD_LDS_BUDGET is refused.  The budget is a CU's whole LDS; the largest launch the tests make takes 162 932
 * bytes of it (139 rows with the full band).  Above 64 KB the call raises the kernel's dynamic-LDS limit first; should the
 * runtime refuse that, the call returns its HIP error code (positive), launches nothing and leaves the outputs untouched.  OUTPUTS, in the caller's node and pipe order: pressure float[S][N] =
 * (float)(head - elevation); head double[S][N] or NULL; flow double[S][P] or NULL; status int32[S][GATRES_HYD_STATUS] =
 * {iterations used, converged, failed, 0}; final_dq double[S], the last sum |dq| / sum |q| (0 where both are 0).
 * FAILED: a non-finite demand at a junction, fixed head at a fixed node, or a roughness that is not positive and finite; a pivot
 * that is not positive and finite; a non-finite sum in the stop rule; static arrays that are not what is stated above (an end
 * node outside [0, N), a pipe from a node to itself, order / position no permutation pair, a junction pair wider than W).  A
 * failed scenario gets NaN in pressure, head, flow and final_dq, status {iterations so far, 0, 1, 0}, and the next scenario is
 * taken: every loop is bounded by max_iter, N, P and W and every index is checked, whatever the inputs hold.
 * GATRES_E_BADARG before any launch: a NULL pointer other than head or flow; S, N or P < 1; N < 2; W outside [1, N - 1]; the LDS
 * need above; max_iter < 1; accuracy not positive and finite; a stride other than 0 or N; an output overlapping an input or
 * another output. */
#define GATRES_HYD_STATUS 4
#define GATRES_HYD_LDS_BUDGET 163840
#define GATRES_HYD_GRID_CAP 1024
int gatres_hydraulic_draw(const double* d_lo, const double* d_hi, const double* c_lo, const double* c_hi, int64_t num_scenarios,
                          int32_t num_nodes, int32_t num_pipes, uint64_t seed, int64_t first_scenario, double* demand,
                          double* roughness, void* stream);
int gatres_hydraulic_solve(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                           const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                           int32_t half_bandwidth, const double* demand, const double* roughness, const double* fixed_head,
                           int64_t fixed_head_stride, int64_t num_scenarios, int32_t num_nodes, int32_t num_pipes, double accuracy,
                           int32_t max_iter, float* pressure, double* head, double* flow, int32_t* status, double* final_dq,
                           void* stream);

/* valid[s] (device uint8) = 1 iff status[s] says converged and not failed and pressure[s][i] lies in [p_lo, p_hi] (compared in
 * fp64; a NaN lies outside) at every junction i (fixed[i] == 0); else 0.  One wave per scenario on a capped grid.
 * GATRES_E_BADARG before any launch: a NULL pointer; num_scenarios or num_nodes < 1; p_lo or p_hi NaN, or p_lo > p_hi; valid
 * overlapping an input. */
int gatres_hydraulic_valid(const float* pressure, const int32_t* status, const uint8_t* fixed, int64_t num_scenarios,
                           int32_t num_nodes, double p_lo, double p_hi, uint8_t* valid, void* stream);

/* THE SERIES: extended-period simulation (symbols only: the ABI stays; k_hydraulics.hip, hydraulics.py).  A series is T steps of
 * dt seconds of one scenario.  TANKS are K of the fixed-head nodes: tank k sits at node tank_node[k], its bottom at that node's
 * elevation, with the area A_k = pi D_k^2 / 4 (tank_area, formed by the caller) and the level limits tank_min_level[k] <=
 * tank_max_level[k] (the maximum may be +infinity: a tank that is never full).  During step t its head is
 * elevation + level[t][k], one fp64 add.  RESERVOIRS are the other fixed-head nodes; they keep fixed_head for the whole series.
 * DEMAND: junction n of series s draws demand[s][n] * mult[pattern_of_node[n]][t] at step t, one rounded fp64 product that is
 * stored before the assembly reads it.  mult is double[M][T] for every series (mult_stride 0) or double[S][M][T] (mult_stride
 * M * T); pattern_of_node int32[N] holds values in [0, M) (read at every node).  A STEP is the steady solve stated above: the
 * same law, assembly, factorisation, flow update and stop rule, one function in k_hydraulics_dev.h for both kernels.  Step 0
 * starts from q_start; step t > 0 starts from the final flows of step t - 1 where warm_start != 0 (EPANET's way), else from
 * q_start again.  LEVEL UPDATE, explicit Euler as in EPANET, after step t, one thread per tank:
 *   inflow_k = 0;  for p = 0 .. P - 1:  inflow_k += q_p where pipe_b[p] is the tank,  inflow_k -= q_p where pipe_a[p] is the tank;
 *   v = inflow_k * dt;   l = level[t][k] + v / A_k;   level[t + 1][k] = min_level[k] if l < min_level[k], max_level[k] if
 *   l > max_level[k], else l
 * with every operation rounded to fp64 on its own.  level[0] is initial_level as given.
 * WHAT DOES NOT HOLD: EPANET shortens a time step at the moment a tank becomes full or empty and closes the pipes of such a
 * tank; this model clamps the level and does neither.  A step after which a level was clamped gets status[s][t][3] = 1, and
 * volume is not conserved across it.  Pumps, check valves, closed links and minor losses are the matter of THE LINK LAW below
 * (gatres_hydraulic_series_links), PRV and PSV valves of THE REGULATING VALVES (gatres_hydraulic_series_valves); simple controls
 * of THE CONTROLS (gatres_hydraulic_series_controls); rules are not modelled.  The limit on flows that
 * should be zero carries over: a step with a zero multiplier does not meet the stop rule.
 * FAILURE: a step fails on a multiplier of the step (any of the M) that is negative or not finite, a product demand * mult or
 * a tank head that is not finite, a pivot that is not positive and finite or a non-finite sum of the stop rule; a series fails
 * from step 0 on a roughness that is not positive and finite or a non-finite fixed_head at a fixed node (tanks included: the
 * value is read and then replaced).  Once a step has failed, it and every later step of the series are failed: pressure, head,
 * flow, final_dq of those steps and level[t + 1] are NaN, status {iterations so far, 0, 1, 0}; the earlier steps keep their
 * outputs.  A step that does not converge is no failure: the series goes on from its flows and heads with converged = 0.  Static
 * arrays that are not what is stated (those of gatres_hydraulic_solve; a tank node outside [0, N), not fixed or listed twice; an
 * area that is not positive and finite; min > max or a NaN limit; a pattern index outside [0, M)) fail every series of the launch.
 *
 * gatres_hydraulic_series: one workgroup of 256 threads per series on a grid capped at GATRES_HYD_GRID_CAP, the series beyond
 * it taken by a loop; the band stays in LDS for the whole series and nothing goes to the host between steps.  LDS need:
 *   the bytes of gatres_hydraulic_solve  +  8 N (the step's demand)  +  40 K (levels, area, two limits, node and row per tank)
 * refused above GATRES_HYD_LDS_BUDGET (hydraulics.series_lds_bytes restates it).  Inputs as for gatres_hydraulic_solve, and
 * tank_node int32[K], tank_area, tank_min_level, tank_max_level double[K], initial_level double[S][K].  OUTPUTS:
 * pressure float[S][T][N]; head double[S][T][N] or NULL; flow double[S][T][P] or NULL; level double[S][T + 1][K];
 * status int32[S][T][GATRES_HYD_STATUS] = {iterations, converged, failed, a level was clamped}; final_dq double[S][T].  No
 * atomics; every sum runs in a fixed order; a series' bits depend on nothing but its own inputs.  K == 0 is legal (patterns
 * only): the tank arrays, initial_level and level may then be NULL.
 * GATRES_E_BADARG before any launch: a NULL pointer other than head or flow (and, with K == 0, the tank arrays); S, T, N, P or
 * M < 1; N < 2; K < 0; W outside [1, N - 1]; dt, accuracy not positive and finite; max_iter < 1; mult_stride neither 0 nor
 * M * T; fixed_head_stride neither 0 nor N; byte counts that do not fit in 64 bits; the LDS need above; an output overlapping
 * an input or another output. */
int gatres_hydraulic_series(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                            const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                            int32_t half_bandwidth, const int32_t* tank_node, const double* tank_area,
                            const double* tank_min_level, const double* tank_max_level, int32_t num_tanks,
                            const int32_t* pattern_of_node, const double* mult, int64_t mult_stride, int32_t num_patterns,
                            const double* demand, const double* roughness, const double* fixed_head, int64_t fixed_head_stride,
                            const double* initial_level, int64_t num_series, int32_t num_steps, int32_t num_nodes,
                            int32_t num_pipes, double dt, int32_t warm_start, double accuracy, int32_t max_iter, float* pressure,
                            double* head, double* flow, double* level, int32_t* status, double* final_dq, void* stream);

/* valid[s] (device uint8) = 1 iff every step of series s converged and none failed, no step has status[s][t][3] != 0 (unless
 * allow_limited != 0) and pressure[s][t][i] lies in [p_lo, p_hi] (compared in fp64; a NaN lies outside) at every junction i of
 * every step; else 0.  One wave per series on a capped grid.  GATRES_E_BADARG before any launch: a NULL pointer; num_series,
 * num_steps or num_nodes < 1; byte counts that do not fit; p_lo or p_hi NaN, or p_lo > p_hi; valid overlapping an input. */
int gatres_hydraulic_series_valid(const float* pressure, const int32_t* status, const uint8_t* fixed, int64_t num_series,
                                  int32_t num_steps, int32_t num_nodes, double p_lo, double p_hi, int32_t allow_limited,
                                  uint8_t* valid, void* stream);

/* THE LINK LAW: pumps, check valves, closed links and minor losses (symbols only: the ABI stays; k_hydraulic_links.hip,
 * hydraulics.py).  The two launches below are gatres_hydraulic_solve and gatres_hydraulic_series with one thing replaced: the law
 * h_p(q), g_p(q) of a link.  Every link p has a KIND, link_kind[p] = GATRES_HYD_PIPE or GATRES_HYD_PUMP, and FLAGS, link_flags[p],
 * a sum of GATRES_HYD_LINK_CHECK (flow only from a_p to b_p) and GATRES_HYD_LINK_CLOSED.  A pump is always CHECK.  The law gives
 * the head loss H_a - H_b = h_p(q) and its gradient g_p, every operation rounded to fp64 on its own:
 *   PIPE, forward branch:   h = r |q|^0.852 q + m |q| q,   g = 1.852 r |q|^0.852 + 2 m |q|,   formed as
 *     ra = r * pow(|q|, 0.852);  ma = m * |q|;  g = 1.852 * ra + 2 * ma;  h = (ra + ma) * q;   where g < 1e-7:  g = 1e-7, h = 1e-7 * q
 *     (the law at low flow).  m = minor[p] = 8 K / (pi^2 * 9.80665 * D^4) is formed by the caller from the minor-loss coefficient
 *     K; m = 0 is the pipe of THE MODEL in every bit; r = 0 (coef = 0) with m > 0 is allowed, a throttle valve (EPANET's TCV).
 *   PUMP k, forward branch (q >= 0): speed w, shut-off head h0 >= 0, coefficient rp > 0, exponent n >= 1; by the affinity laws
 *     the head gain is w^2 h0 - w^(2-n) rp q^n, so   h = -w^2 h0 + w^(2-n) rp q^n,   g = n w^(2-n) rp q^(n-1),   formed as
 *     ca = (w2n * rp) * pow(q, n - 1);  g = n * ca;  hq = ca * q;   where g < 1e-7:  g = 1e-7, hq = 1e-7 * q;   h = hq - w2 * h0
 *     with w2 = w * w and w2n = pow(w, 2 - n) formed once per scenario (or step) and pump.  A pump's coef and roughness are not read.
 *   REVERSE BRANCH of a CHECK link (q < 0):   g = 1e8,   h = h(0) + 1e8 q,   h(0) = 0 for a pipe and -w2 * h0 for a pump.
 *   A CLOSED link -- by its flag, by the scenario's byte closed[s][p] = 1, or a pump with w == 0:   g = 1e8,   h = 1e8 q at every q;
 *     such a link starts at q = 0 (in a series at every step in which it is shut, warm start or not).
 * The law is continuous and monotone in q, up to the jump at the low-flow floor that THE MODEL already has, so the system stays
 * symmetric positive definite and the solution unique.  THERE IS NO STATUS MACHINE: a link that holds shut carries -dh / 1e8, as a
 * closed link does in EPANET.  Assembly, factorisation, flow update and stop rule are those of THE SOLVER, the same function
 * (hy_newton in k_hydraulics_dev.h) with the law chosen at compile time.  New output link_state uint8[S][P] (series: [S][T][P]),
 * evaluated at the returned flows: 0 forward; 1 a CHECK link on its reverse branch (q < 0); 2 shut by input or by w == 0; 0
 * where the scenario or step failed.
 * WHAT DOES NOT HOLD: a zone that CHECK or shut links cut off from every fixed-head node gets heads near -1e8 x demand and
 * usually does not meet the stop rule; such scenarios are counted and dropped by the generators, never repaired.
 * PRV and PSV valves are the matter of THE REGULATING VALVES below, which do have one; PBV, FCV and GPV valves, power-rated pumps,
 * and rule-based controls stay out of scope (simple controls: THE CONTROLS).  Parity with EPANET is not claimed and has not been checked.
 * STATIC link inputs (device): link_kind, link_flags uint8[P]; minor double[P]; pump_link int32[Kp], the link of pump k;
 * pump_h0, pump_r, pump_n double[Kp].  Kp == 0 is legal, the pump arrays and speed may then be NULL.  PER-SCENARIO: speed
 * double, row s at speed + s * speed_stride, speed_stride 0 or Kp; closed uint8 or NULL, row s at closed + s * closed_stride,
 * closed_stride 0 or P.  In the series the speed of pump k in step t is speed[s][k] * speed_mult[speed_pattern_of_pump[k]][t],
 * one rounded product, speed_mult double[Ms][T]; 0 is legal: the pump is off in that step.
 * FAILED, every scenario of the launch: a kind above 1, flags above 3, m negative or not finite, a pipe's coef negative, not
 * finite, or 0 with m = 0; pump_link outside [0, P), on a link that is no pump or listed twice, a pump link without a pump;
 * h0 < 0, rp <= 0, n < 1 or any of them not finite; in the series a speed pattern outside [0, Ms).  That scenario (in the series
 * that step and the later ones) alone: a speed, or in the series a speed multiplier of the step, that is negative or not finite,
 * a w^2 or w^(2-n) that is not finite, a closed byte above 1, and what fails a scenario of gatres_hydraulic_solve (a pipe's
 * r = 0 fails only where m = 0).
 * LDS need (hydraulics.links_lds_bytes, series_links_lds_bytes): the bytes of gatres_hydraulic_solve (of gatres_hydraulic_series)
 *   + 12 P (m and the link's code)  +  48 Kp (h0, rp, n, w^2, w^(2-n), w per pump),
 * refused above GATRES_HYD_LDS_BUDGET.  The 12 P bytes are taken whether or not a link is special, so a pipe-only network whose
 * band leaves fewer than 12 P bytes of the budget runs through gatres_hydraulic_solve and is refused here (a full band of 139
 * rows is such a network).
 * GATRES_E_BADARG before any launch: what gatres_hydraulic_solve (gatres_hydraulic_series) refuses; link_kind, link_flags, minor
 * or link_state NULL; Kp < 0 or Kp > P; Kp > 0 with a NULL pump array or speed (in the series: speed_mult or
 * speed_pattern_of_pump NULL, or Ms < 1); Ms < 0; speed_stride neither 0 nor Kp; closed_stride neither 0 nor P, or not 0 with
 * closed NULL; the LDS need above; an output, link_state included, overlapping an input or another output. */
#define GATRES_HYD_PIPE 0
#define GATRES_HYD_PUMP 1
#define GATRES_HYD_LINK_CHECK 1
#define GATRES_HYD_LINK_CLOSED 2
int gatres_hydraulic_solve_links(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                 const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                 int32_t half_bandwidth, const double* demand, const double* roughness, const double* fixed_head,
                                 int64_t fixed_head_stride, int64_t num_scenarios, int32_t num_nodes, int32_t num_pipes,
                                 double accuracy, int32_t max_iter, float* pressure, double* head, double* flow, int32_t* status,
                                 double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags, const double* minor,
                                 const int32_t* pump_link, const double* pump_h0, const double* pump_r, const double* pump_n,
                                 int32_t num_pumps, const double* speed, int64_t speed_stride, const uint8_t* closed,
                                 int64_t closed_stride, uint8_t* link_state, void* stream);
int gatres_hydraulic_series_links(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                  const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                  int32_t half_bandwidth, const int32_t* tank_node, const double* tank_area,
                                  const double* tank_min_level, const double* tank_max_level, int32_t num_tanks,
                                  const int32_t* pattern_of_node, const double* mult, int64_t mult_stride, int32_t num_patterns,
                                  const double* demand, const double* roughness, const double* fixed_head,
                                  int64_t fixed_head_stride, const double* initial_level, int64_t num_series, int32_t num_steps,
                                  int32_t num_nodes, int32_t num_pipes, double dt, int32_t warm_start, double accuracy,
                                  int32_t max_iter, float* pressure, double* head, double* flow, double* level, int32_t* status,
                                  double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags, const double* minor,
                                  const int32_t* pump_link, const double* pump_h0, const double* pump_r, const double* pump_n,
                                  int32_t num_pumps, const double* speed, int64_t speed_stride, const uint8_t* closed,
                                  int64_t closed_stride, const double* speed_mult, const int32_t* speed_pattern_of_pump,
                                  int32_t num_speed_patterns, uint8_t* link_state, void* stream);

/* THE REGULATING VALVES: pressure-reducing (PRV) and pressure-sustaining (PSV) valves, with a status machine (symbols only: the
 * ABI stays; k_hydraulic_network.hip, hydraulics.py).  The two launches below are gatres_hydraulic_solve_links and
 * gatres_hydraulic_series_links with link_kind values GATRES_HYD_PRV and GATRES_HYD_PSV allowed; the links launches refuse them as
 * they always did.  A regulating valve is a link from a to b without pipe resistance (r = 0: its coef and roughness are not read,
 * as for a pump) and with the minor-loss term m = minor[p] of any link (m = 0 is allowed).  It has a setting s, a pressure in
 * metres, and one CONTROLLED NODE c:  PRV: c = b, the downstream end;  PSV: c = a, the upstream end.  Its target head is
 * hset = elevation[c] + s, one fp64 add.  During the Newton loop it carries a STATUS, OPEN, ACTIVE or CLOSED; it starts ACTIVE.
 * LAW BY STATUS.  OPEN: the PIPE branch of THE LINK LAW with r = 0 (where g < 1e-7 the linear floor, so m = 0 is a valve that loses
 * nothing).  CLOSED: g = 1e8, h = 1e8 q.  ACTIVE: the link is not in the matrix at all.
 * ASSEMBLY WITH ACTIVE VALVES.  The controlled node of an ACTIVE valve is a fixed-head row at hset for that iteration: its row is
 * the identity row that a reservoir's is, its neighbours take pi * hset on their right-hand side, and no off-diagonal is written
 * for it, so the band never widens.  The valve's present flow q_v is a fixed draw: -q_v on the right-hand side of row a and +q_v
 * on that of row b, wherever that row is neither fixed nor the controlled node of an ACTIVE valve; it takes its place in the
 * row's sum in pipe order.
 * FLOWS.  After the head solve every link that is not an ACTIVE valve updates as in THE SOLVER.  Each ACTIVE valve then takes the
 * flow that closes the mass balance at c over the other links' new flows, added up in pipe order (+q_p where link p ends at c,
 * -q_p where it starts there):  PRV: q_v = d_c - inflow;  PSV: q_v = inflow - d_c;  its dq is old flow - new flow.
 * STATUS.  Every valve reads the new heads H_a, H_b and its own new q, all valves from the old statuses at once, with
 * HTOL = 1.524e-4 m and QTOL = 2.8316846592e-6 m3/s (EPANET's 0.0005 ft and 0.0001 cfs) and hml = (m * |q|) * q:
 *   PRV ACTIVE:  q < -QTOL -> CLOSED;  else H_a - hml < hset - HTOL -> OPEN;  else ACTIVE
 *   PRV OPEN:    q < -QTOL -> CLOSED;  else H_b >= hset + HTOL -> ACTIVE;  else OPEN
 *   PRV CLOSED:  H_a >= hset + HTOL and H_b < hset - HTOL -> ACTIVE;  else H_a < hset - HTOL and H_a > H_b + HTOL -> OPEN;  else CLOSED
 *   PSV ACTIVE:  q < -QTOL -> CLOSED;  else H_b + hml > hset + HTOL -> OPEN;  else ACTIVE
 *   PSV OPEN:    q < -QTOL -> CLOSED;  else H_a < hset - HTOL -> ACTIVE;  else OPEN
 *   PSV CLOSED:  H_b > hset + HTOL and H_a > H_b + HTOL -> OPEN;  else H_a >= hset + HTOL and H_a > H_b + HTOL -> ACTIVE;  else CLOSED
 * A valve that turns CLOSED gets q = 0.
 * STOP RULE.  sum |dq| <= accuracy * sum |q| AND no status changed in this iteration; the dq of a valve that has just closed is
 * the one from before it was zeroed, the q in the sum the one after.
 * SHUT VALVES.  A valve shut by GATRES_HYD_LINK_CLOSED or by closed[s][p] = 1 is a shut link of THE LINK LAW (link_state 2) and its
 * status machine does not run.  link_state of a regulating valve otherwise: 0 OPEN, 3 ACTIVE, 4 CLOSED by its own status.
 * SERIES.  With warm_start the statuses carry over from step to step along with the flows; without it they start ACTIVE at every
 * step.  Settings do not follow patterns.
 * WHAT DOES NOT HOLD: the valve's flow lags one iteration behind the heads, as in EPANET, so convergence across a valve is linear,
 * not quadratic.  Statuses can cycle: such a scenario uses all its iterations, is not converged, and is dropped by
 * gatres_hydraulic_valid, never repaired.  An OPEN valve with m = 0 sits on the linear floor (1 / g = 1e7): its flow moves by
 * 1e-7 m3/s per ulp of the heads, as THE MODEL says of every flow on that branch, and whether such a scenario meets the stop rule
 * is decided by rounding; give a valve a loss coefficient where that matters.  Parity with EPANET is not claimed.  FCV, PBV, GPV, power-rated pumps and rule-based
 * controls stay out of scope.  The ACTIVE system is singular unless, with all regulating valves removed, the uncontrolled end of every valve
 * still reaches a fixed-head node and every junction reaches a fixed-head node or the controlled node of some valve; the caller
 * sees to that (hydraulics.HydraulicNetwork refuses other networks), and a scenario that still produces a bad pivot fails.
 * INPUTS after those of the links launches: valve_link int32[Kv], the link of valve k; valve_kind uint8[Kv], GATRES_HYD_PRV or
 * GATRES_HYD_PSV; valve_setting double, row s at valve_setting + s * valve_setting_stride, the stride 0 or Kv; Kv == 0 is legal (the
 * three may be NULL), and the launch then gives every bit of the links launch.  OUTPUT valve_changes int32[S] (series: [S][T]):
 * the status changes of the scenario or step over all its iterations, 0 where it failed.
 * FAILED, every scenario of the launch: what fails every scenario of the links launches, with kinds up to GATRES_HYD_PSV allowed; a
 * valve link with the CHECK flag; valve_link outside [0, P), on a link whose kind is not valve_kind[k], or listed twice; a link of
 * kind PRV or PSV without a valve; two valves that share a node; a controlled node that is a fixed-head node.  That scenario (in
 * the series that step and the later ones) alone: a setting or an hset that is not finite.
 * LDS need (hydraulics.valves_lds_bytes, series_valves_lds_bytes): the bytes of gatres_hydraulic_solve_links (of
 * gatres_hydraulic_series_links)  +  24 Kv (hset, link, row and node of c, change flag per valve), refused above
 * GATRES_HYD_LDS_BUDGET.
 * GATRES_E_BADARG before any launch: what the links launches refuse; valve_changes NULL; Kv < 0 or Kv > P; Kv > 0 with a NULL
 * valve array; valve_setting_stride neither 0 nor Kv; the LDS need above; an output, valve_changes included, overlapping an input
 * or another output. */
#define GATRES_HYD_PRV 2
#define GATRES_HYD_PSV 3
int gatres_hydraulic_solve_valves(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                  const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                  int32_t half_bandwidth, const double* demand, const double* roughness, const double* fixed_head,
                                  int64_t fixed_head_stride, int64_t num_scenarios, int32_t num_nodes, int32_t num_pipes,
                                  double accuracy, int32_t max_iter, float* pressure, double* head, double* flow, int32_t* status,
                                  double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags, const double* minor,
                                  const int32_t* pump_link, const double* pump_h0, const double* pump_r, const double* pump_n,
                                  int32_t num_pumps, const double* speed, int64_t speed_stride, const uint8_t* closed,
                                  int64_t closed_stride, uint8_t* link_state, const int32_t* valve_link, const uint8_t* valve_kind,
                                  const double* valve_setting, int64_t valve_setting_stride, int32_t num_valves,
                                  int32_t* valve_changes, void* stream);
int gatres_hydraulic_series_valves(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                   const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                   int32_t half_bandwidth, const int32_t* tank_node, const double* tank_area,
                                   const double* tank_min_level, const double* tank_max_level, int32_t num_tanks,
                                   const int32_t* pattern_of_node, const double* mult, int64_t mult_stride, int32_t num_patterns,
                                   const double* demand, const double* roughness, const double* fixed_head,
                                   int64_t fixed_head_stride, const double* initial_level, int64_t num_series, int32_t num_steps,
                                   int32_t num_nodes, int32_t num_pipes, double dt, int32_t warm_start, double accuracy,
                                   int32_t max_iter, float* pressure, double* head, double* flow, double* level, int32_t* status,
                                   double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags, const double* minor,
                                   const int32_t* pump_link, const double* pump_h0, const double* pump_r, const double* pump_n,
                                   int32_t num_pumps, const double* speed, int64_t speed_stride, const uint8_t* closed,
                                   int64_t closed_stride, const double* speed_mult, const int32_t* speed_pattern_of_pump,
                                   int32_t num_speed_patterns, uint8_t* link_state, const int32_t* valve_link,
                                   const uint8_t* valve_kind, const double* valve_setting, int64_t valve_setting_stride,
                                   int32_t num_valves, int32_t* valve_changes, void* stream);

/* THE EMITTERS: pressure-dependent outflow at junctions, EPANET's emitter q = C p^gamma -- a leak (symbols only: the ABI stays;
 * k_hydraulic_network.hip, hydraulics.py).  The two launches below are gatres_hydraulic_solve_valves and
 * gatres_hydraulic_series_valves with a node term for Ke emitters.  Emitter k sits on junction i = emitter_node[k].  It has a
 * coefficient C >= 0 (m3/s per m^gamma) per scenario and emitter, and the launch has one exponent gamma.  It is a virtual link
 * from i to the fixed head z_i = elevation[i] with a flow q_e of its own, positive out of the network.  With n = 1 / gamma and
 * ce = pow(C, -n), both formed once per scenario (in a series: per step) and emitter:
 * FORWARD BRANCH (q_e >= 0): ca = ce * pow(q_e, n - 1), g = n * ca, h = ca * q_e (h = ce q_e^n).  Where g < 1e-7 the linear floor
 * of THE MODEL applies (g = 1e-7, h = 1e-7 q_e).  Where g > 1e8 or g is not finite (q_e -> 0 with gamma > 1; a ce that overflowed):
 * g = 1e8, h = 1e8 q_e.
 * REVERSE BRANCH (q_e < 0): a leak takes no water in: g = 1e8, h = 1e8 q_e, the reverse branch of a CHECK link.  A junction under
 * negative pressure p therefore carries -|p| / 1e8, as every shut link of this solver does.
 * C == 0 in a scenario or step means no emitter there: its row gets nothing, q_e is +0.0, and it adds nothing to the sums of the
 * stop rule.
 * ASSEMBLY.  Row of i, after the row's sum over the links in pipe order, with 1 / g formed once:  diag += 1 / g;
 * f -= q_e - h / g;  f += z_i * (1 / g).  No off-diagonal is written, so the band never widens.
 * FLOW UPDATE, after the links':  dq = h / g - (H_i - z_i) * (1 / g);  q_e -= dq.
 * STOP RULE.  |dq| and |q_e| of the emitters that are on join the two sums after the links, in emitter order, added by the same
 * thread.
 * START.  q_e = C, the flow at one metre of pressure.
 * SERIES.  emitter_onset int32, row s at emitter_onset + s * emitter_onset_stride (stride 0 or Ke; NULL: all 0): emitter k has
 * C = 0 at the steps t < onset[k]; this is how a leak begins in the middle of a series.  With warm_start an emitter that was on in
 * the step before keeps its q_e; one that has just switched on, and every emitter without warm_start, starts at C.
 * WHAT DOES NOT HOLD: an emitter on the controlled node of a regulating valve is refused, not modelled: an ACTIVE valve closes
 * the mass balance at that node over the links alone, and that rule stays as it stands.  Pressure-driven demand (EPANET 2.2's
 * DEMAND MODEL PDA) takes the same node slot, at every junction that draws: THE PRESSURE-DRIVEN DEMAND, below.  Parity with
 * EPANET is not claimed.
 * INPUTS after those of the valves launches: emitter_node int32[Ke]; emitter_coef double, row s at emitter_coef + s *
 * emitter_coef_stride, the stride 0 or Ke; num_emitters = Ke; emitter_exponent = gamma; (series) emitter_onset and its stride.
 * Ke == 0 is legal (the arrays may be NULL), and the launch then gives every bit of the valves launch.  OUTPUT emitter_flow
 * double[S][Ke] (series: [S][T][Ke]) at the returned heads' iteration, as flow is; NaN where the scenario or step failed.
 * FAILED, every scenario of the launch: what fails every scenario of the valves launches; gamma not finite, not positive, or with
 * 1 / gamma not finite; an emitter node outside [0, N), listed twice, a fixed-head node, or the controlled node of a regulating
 * valve.  That scenario alone: a C that is negative or not finite (a series with such a C fails from step 0 on, whatever the
 * onset).
 * LDS need (hydraulics.emitters_lds_bytes, series_emitters_lds_bytes): the bytes of gatres_hydraulic_solve_valves (of
 * gatres_hydraulic_series_valves)  +  48 Ke (ce, z, q_e, 1 / g, h / g, row and node per emitter), refused above
 * GATRES_HYD_LDS_BUDGET.
 * GATRES_E_BADARG before any launch: what the valves launches refuse; Ke < 0 or Ke > N; Ke > 0 with emitter_node, emitter_coef or
 * emitter_flow NULL; emitter_coef_stride neither 0 nor Ke; emitter_onset_stride neither 0 nor Ke, or Ke with emitter_onset NULL;
 * the LDS need above; an output, emitter_flow included, overlapping an input or another output. */
int gatres_hydraulic_solve_emitters(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                    const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                    int32_t half_bandwidth, const double* demand, const double* roughness, const double* fixed_head,
                                    int64_t fixed_head_stride, int64_t num_scenarios, int32_t num_nodes, int32_t num_pipes,
                                    double accuracy, int32_t max_iter, float* pressure, double* head, double* flow, int32_t* status,
                                    double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags, const double* minor,
                                    const int32_t* pump_link, const double* pump_h0, const double* pump_r, const double* pump_n,
                                    int32_t num_pumps, const double* speed, int64_t speed_stride, const uint8_t* closed,
                                    int64_t closed_stride, uint8_t* link_state, const int32_t* valve_link,
                                    const uint8_t* valve_kind, const double* valve_setting, int64_t valve_setting_stride,
                                    int32_t num_valves, int32_t* valve_changes, const int32_t* emitter_node,
                                    const double* emitter_coef, int64_t emitter_coef_stride, int32_t num_emitters,
                                    double emitter_exponent, double* emitter_flow, void* stream);
int gatres_hydraulic_series_emitters(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                     const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                     int32_t half_bandwidth, const int32_t* tank_node, const double* tank_area,
                                     const double* tank_min_level, const double* tank_max_level, int32_t num_tanks,
                                     const int32_t* pattern_of_node, const double* mult, int64_t mult_stride, int32_t num_patterns,
                                     const double* demand, const double* roughness, const double* fixed_head,
                                     int64_t fixed_head_stride, const double* initial_level, int64_t num_series, int32_t num_steps,
                                     int32_t num_nodes, int32_t num_pipes, double dt, int32_t warm_start, double accuracy,
                                     int32_t max_iter, float* pressure, double* head, double* flow, double* level, int32_t* status,
                                     double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags, const double* minor,
                                     const int32_t* pump_link, const double* pump_h0, const double* pump_r, const double* pump_n,
                                     int32_t num_pumps, const double* speed, int64_t speed_stride, const uint8_t* closed,
                                     int64_t closed_stride, const double* speed_mult, const int32_t* speed_pattern_of_pump,
                                     int32_t num_speed_patterns, uint8_t* link_state, const int32_t* valve_link,
                                     const uint8_t* valve_kind, const double* valve_setting, int64_t valve_setting_stride,
                                     int32_t num_valves, int32_t* valve_changes, const int32_t* emitter_node,
                                     const double* emitter_coef, int64_t emitter_coef_stride, int32_t num_emitters,
                                     double emitter_exponent, const int32_t* emitter_onset, int64_t emitter_onset_stride,
                                     double* emitter_flow, void* stream);

/* THE PRESSURE-DRIVEN DEMAND: EPANET 2.2's DEMAND MODEL PDA (symbols only: the ABI stays; k_hydraulic_network.hip, hydraulics.py).
 * The two launches below are gatres_hydraulic_solve_emitters and gatres_hydraulic_series_emitters with a node term for the
 * demand.  A launch has demand_model (0 demand-driven, 1 pressure-driven) and three scalars: minimum_pressure Pmin and
 * required_pressure Preq in metres, pressure_exponent e (EPANET's default 0.5).  dp = Preq - Pmin, n = 1 / e.
 * WHICH JUNCTIONS.  Junction i is pressure-driven in a scenario (in a series: in a step) where its full demand D_i is positive;
 * D_i is demand[i], in a series the step's rounded product demand[i] * multiplier.  A junction with D_i <= 0 (an inflow
 * included) and every fixed-head node keep the fixed draw -demand exactly as in the emitters launches.
 * THE VIRTUAL LINK.  A pressure-driven junction is a virtual link from i to the fixed head z_i = elevation[i] + Pmin with a flow
 * q_d of its own, positive out of the network.  Its law (EPANET 2.2's demandheadloss with this solver's gradients 1e8 and 1e-7):
 *   q_d < 0:        g = 1e8, h = 1e8 q_d: no demand node feeds the network.
 *   0 <= q_d <= D:  g = ((n * dp) * pow(q_d / D, n - 1)) / D, h = (g * q_d) / n, which is dp (q_d / D)^n.  Where g < 1e-7 the linear
 *                   floor of THE MODEL applies (g = 1e-7, h = 1e-7 q_d).  Where g > 1e8 or g is not finite: g = 1e8, h = 1e8 q_d.
 *   q_d > D:        g = 1e8, h = dp + 1e8 (q_d - D).  A junction above Preq delivers D + (p - Preq) / 1e8, as every shut link of
 *                   this solver leaks; a junction below Pmin carries -|p - Pmin| / 1e8.
 * ASSEMBLY.  For a pressure-driven row the term -demand is not added (f starts at 0).  After the row's links in pipe order and
 * after an emitter's term, with 1 / g formed once:  diag += 1 / g;  f -= q_d - h / g;  f += z_i * (1 / g).  No off-diagonal is
 * written, so the band never widens.
 * FLOW UPDATE, after the links' and the emitters':  dq = h / g - (H_i - z_i) * (1 / g);  q_d -= dq.
 * STOP RULE.  |dq| and |q_d| of the pressure-driven junctions join the two sums after the links and the emitters, in node order,
 * added by the same thread.  (The kernel adds the +0.0 that the other nodes hold in the same arrays, which changes no bit.)
 * START.  q_d = D.
 * SERIES.  D changes with the multipliers.  With warm_start a junction that was pressure-driven in the step before keeps its
 * q_d; one that has just become pressure-driven, and every junction without warm_start, starts at D.  The tank levels follow the
 * link flows as they always did, so a starved network drains its tanks more slowly.
 * REGULATING VALVES.  The controlled node of a regulating valve may be pressure-driven.  While the valve is ACTIVE the row is
 * the identity row it always was, the virtual link's flow update still runs from the row's head (the valve's target), and the
 * valve's thread closes the mass balance of the node with the junction's new q_d where it reads the demand otherwise.  An
 * emitter on such a node stays refused.
 * EMITTERS.  An emitter and pressure-driven demand may share a junction; both terms add, the emitter's first.
 * INPUTS after those of the emitters launches: demand_model, minimum_pressure, required_pressure, pressure_exponent.  OUTPUT
 * demand_delivered double[S][N] (series: [S][T][N]): q_d at a pressure-driven junction, the demand itself (the step's product) at
 * another junction, 0 at a fixed-head node; at the returned heads' iteration, as flow is; NaN where the scenario or step failed.
 * pressure, head, flow, status, link_state, valve_changes and emitter_flow keep their meaning.
 * With demand_model 0 the launch gives every bit of the emitters launch on the same inputs; the three scalars are not read, and
 * demand_delivered may be NULL (where it is not, it gets the demands as said above).
 * FAILED, every scenario of the launch: what fails every scenario of the emitters launches; with demand_model 1, Pmin or Preq
 * not finite, dp < 0.1 m (EPANET's MINPDIFF) or not a number, e or 1 / e not finite or not positive.  That scenario or step alone
 * (a series: from that step on): a pressure-driven junction whose elevation + Pmin is not finite.
 * LDS need (hydraulics.pdd_lds_bytes, series_pdd_lds_bytes): the bytes of gatres_hydraulic_solve_emitters (of
 * gatres_hydraulic_series_emitters)  +  with demand_model 1, 32 N (D, q_d, 1 / g and h / g per node; z_i is formed from the
 * elevation where it is used), refused above GATRES_HYD_LDS_BUDGET.  The 388 / 430 / 3 network of the tests takes 104 680 bytes
 * (series: 107 904).
 * GATRES_E_BADARG before any launch: what the emitters launches refuse; demand_model outside {0, 1}; demand_delivered NULL with
 * demand_model 1; the LDS need above; an output, demand_delivered included, overlapping an input or another output. */
int gatres_hydraulic_solve_pdd(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                               const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                               int32_t half_bandwidth, const double* demand, const double* roughness, const double* fixed_head,
                               int64_t fixed_head_stride, int64_t num_scenarios, int32_t num_nodes, int32_t num_pipes,
                               double accuracy, int32_t max_iter, float* pressure, double* head, double* flow, int32_t* status,
                               double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags, const double* minor,
                               const int32_t* pump_link, const double* pump_h0, const double* pump_r, const double* pump_n,
                               int32_t num_pumps, const double* speed, int64_t speed_stride, const uint8_t* closed,
                               int64_t closed_stride, uint8_t* link_state, const int32_t* valve_link,
                               const uint8_t* valve_kind, const double* valve_setting, int64_t valve_setting_stride,
                               int32_t num_valves, int32_t* valve_changes, const int32_t* emitter_node,
                               const double* emitter_coef, int64_t emitter_coef_stride, int32_t num_emitters,
                               double emitter_exponent, double* emitter_flow, int32_t demand_model, double minimum_pressure,
                               double required_pressure, double pressure_exponent, double* demand_delivered, void* stream);
int gatres_hydraulic_series_pdd(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                int32_t half_bandwidth, const int32_t* tank_node, const double* tank_area,
                                const double* tank_min_level, const double* tank_max_level, int32_t num_tanks,
                                const int32_t* pattern_of_node, const double* mult, int64_t mult_stride, int32_t num_patterns,
                                const double* demand, const double* roughness, const double* fixed_head,
                                int64_t fixed_head_stride, const double* initial_level, int64_t num_series, int32_t num_steps,
                                int32_t num_nodes, int32_t num_pipes, double dt, int32_t warm_start, double accuracy,
                                int32_t max_iter, float* pressure, double* head, double* flow, double* level, int32_t* status,
                                double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags, const double* minor,
                                const int32_t* pump_link, const double* pump_h0, const double* pump_r, const double* pump_n,
                                int32_t num_pumps, const double* speed, int64_t speed_stride, const uint8_t* closed,
                                int64_t closed_stride, const double* speed_mult, const int32_t* speed_pattern_of_pump,
                                int32_t num_speed_patterns, uint8_t* link_state, const int32_t* valve_link,
                                const uint8_t* valve_kind, const double* valve_setting, int64_t valve_setting_stride,
                                int32_t num_valves, int32_t* valve_changes, const int32_t* emitter_node,
                                const double* emitter_coef, int64_t emitter_coef_stride, int32_t num_emitters,
                                double emitter_exponent, const int32_t* emitter_onset, int64_t emitter_onset_stride,
                                double* emitter_flow, int32_t demand_model, double minimum_pressure, double required_pressure,
                                double pressure_exponent, double* demand_delivered, void* stream);

/* THE CONTROLS: EPANET's simple controls on pumps, valves and pipes in a series (a symbol only: the ABI stays;
 * k_hydraulic_network.hip, hydraulics.py).  gatres_hydraulic_series_controls is gatres_hydraulic_series_pdd with a table of
 * num_controls = Kc >= 0 controls that switch links by a tank level, a junction pressure or the step's number.  [RULES] stay out.
 * THE TABLE, in an order that matters.  Control k holds
 *   control_link[k]       int32   the controlled link;
 *   control_action[k]     uint8   GATRES_HYD_CTL_OPEN 0, GATRES_HYD_CTL_CLOSED 1, GATRES_HYD_CTL_SETTING 2;
 *   control_value[k]      double  read for SETTING only: on a pump the base speed, in place of speed[s][k'] (the step's
 *                                 speed-pattern multiplier still multiplies it); on a PRV or PSV the setting in metres, in place of
 *                                 valve_setting[s][k'];
 *   control_kind[k]       uint8   GATRES_HYD_CTL_TANK_BELOW 0, TANK_ABOVE 1, NODE_BELOW 2, NODE_ABOVE 3, AT_STEP 4;
 *   control_target[k]     int32   a tank index in [0, K) for kinds 0 and 1, a junction's node index for kinds 2 and 3, a step
 *                                 index for kind 4;
 *   control_threshold     double  [Kc] (control_threshold_stride 0) or [S][Kc] (stride Kc): a level in metres above the tank's
 *                                 bottom for kinds 0 and 1, a pressure in metres for kinds 2 and 3; not read for kind 4.
 * EVALUATION, at the start of step t, before the step's inputs are formed (EPANET's place: between the demands and the solve):
 *   TANK_BELOW  level[t][target] <= threshold;  TANK_ABOVE  >=.  The level the step starts with, so read at t = 0 too.
 *   NODE_BELOW / NODE_ABOVE  H - elevation in fp64 from the solution of step t - 1, <= / >= threshold; not evaluated at t = 0;
 *               evaluated whether or not step t - 1 converged.
 *   AT_STEP     t == target.  A target of T or more never fires.
 * Every control whose condition holds applies its action, in table order, so within a step the last one wins.  Controls are
 * level-triggered, as in EPANET: evaluated at every step, not latched on an edge.
 * STATE.  Each link carries ctl in {none, open, closed} and an override value with a presence flag, reset at the start of every
 * series and kept from step to step until a control changes them.  OPEN sets ctl = open.  CLOSED sets ctl = closed.  SETTING
 * stores the override and sets ctl = open (EPANET: a setting control opens the link).  A control that fires has CHANGED its
 * link when ctl, the presence flag or the bits of the override differ from what they were; control_changes int32 [S][T] counts
 * these per step (0 where the step failed).
 * EFFECT ON THE STEP.  A link is shut by input when ctl == closed, or when ctl == none and the static CLOSED flag or the
 * scenario's closed byte says so; ctl == open overrides both, so a link that starts closed can be opened.  The rule that a pump
 * with w == 0 is shut stands: a SETTING of 0 switches a pump off, and OPEN gives a pump with base speed 0 no speed.  link_state
 * stays as defined; state 2 reads "shut by input, by w == 0 or by a control".  A link with ctl != none that was shut in step
 * t - 1 and is not shut in step t starts step t at q_start[p], warm or cold (a link no control has touched starts as in
 * gatres_hydraulic_series_pdd, which an empty table therefore gives bit for bit); a link that becomes shut starts at 0.  A
 * regulating valve with ctl != none starts the step ACTIVE, even in a warm series, when a control changed its link at step t or
 * when it was shut in step t - 1.
 * FAILED, every series of the launch: what fails every series of gatres_hydraulic_series_pdd; a control whose link is outside
 * [0, P), whose action or kind is unknown, whose link is a CHECK pipe that is no pump (EPANET refuses that too); SETTING on a
 * link that is neither a pump nor a PRV / PSV, with a value that is not finite, or negative on a pump; a tank index outside [0, K);
 * a node of kinds 2 and 3 outside [0, N) or with a fixed head; a negative target.  That series alone, from step 0 on: a threshold
 * of a kind 0 .. 3 control that is not finite.
 * WHAT DOES NOT HOLD.  EPANET shortens a time step so that a level control fires at the moment the level is reached; here levels
 * are read at step starts, so a level overshoots its threshold by up to |inflow| dt / A.  EPANET's volume tolerance on level
 * controls is not modelled.  A control that cuts a zone off from every fixed-head node gives a step that does not converge
 * (gatres_hydraulic_series_valid drops the series, as with the closed bytes).  [RULES] and controls on pipe settings (a TCV's
 * loss, an FCV's flow and the like) stay out of scope.  Parity with EPANET is not claimed.
 * LDS need (hydraulics.series_controls_lds_bytes): the bytes of gatres_hydraulic_series_pdd  +  12 P + 16 (per link the override
 * and the state word; the change counts of the four waves), refused above GATRES_HYD_LDS_BUDGET.
 * GATRES_E_BADARG before any launch: what gatres_hydraulic_series_pdd refuses; num_controls < 0; with num_controls > 0 a NULL
 * table array; control_threshold_stride outside {0, Kc}; control_changes NULL; the LDS need above; an output, control_changes
 * included, overlapping an input or another output.  num_controls == 0 with NULL table arrays is allowed. */
#define GATRES_HYD_CTL_OPEN 0
#define GATRES_HYD_CTL_CLOSED 1
#define GATRES_HYD_CTL_SETTING 2
#define GATRES_HYD_CTL_TANK_BELOW 0
#define GATRES_HYD_CTL_TANK_ABOVE 1
#define GATRES_HYD_CTL_NODE_BELOW 2
#define GATRES_HYD_CTL_NODE_ABOVE 3
#define GATRES_HYD_CTL_AT_STEP 4
int gatres_hydraulic_series_controls(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                     const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                     int32_t half_bandwidth, const int32_t* tank_node, const double* tank_area,
                                     const double* tank_min_level, const double* tank_max_level, int32_t num_tanks,
                                     const int32_t* pattern_of_node, const double* mult, int64_t mult_stride, int32_t num_patterns,
                                     const double* demand, const double* roughness, const double* fixed_head,
                                     int64_t fixed_head_stride, const double* initial_level, int64_t num_series, int32_t num_steps,
                                     int32_t num_nodes, int32_t num_pipes, double dt, int32_t warm_start, double accuracy,
                                     int32_t max_iter, float* pressure, double* head, double* flow, double* level, int32_t* status,
                                     double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags, const double* minor,
                                     const int32_t* pump_link, const double* pump_h0, const double* pump_r, const double* pump_n,
                                     int32_t num_pumps, const double* speed, int64_t speed_stride, const uint8_t* closed,
                                     int64_t closed_stride, const double* speed_mult, const int32_t* speed_pattern_of_pump,
                                     int32_t num_speed_patterns, uint8_t* link_state, const int32_t* valve_link,
                                     const uint8_t* valve_kind, const double* valve_setting, int64_t valve_setting_stride,
                                     int32_t num_valves, int32_t* valve_changes, const int32_t* emitter_node,
                                     const double* emitter_coef, int64_t emitter_coef_stride, int32_t num_emitters,
                                     double emitter_exponent, const int32_t* emitter_onset, int64_t emitter_onset_stride,
                                     double* emitter_flow, int32_t demand_model, double minimum_pressure, double required_pressure,
                                     double pressure_exponent, double* demand_delivered, const int32_t* control_link,
                                     const uint8_t* control_action, const double* control_value, const uint8_t* control_kind,
                                     const int32_t* control_target, const double* control_threshold,
                                     int64_t control_threshold_stride, int32_t num_controls, int32_t* control_changes,
                                     void* stream);

/* THE SENSITIVITIES: first-order sensitivities of the sensor heads and leak localisation (symbols only: the ABI stays;
 * k_hydraulic_sensitivity.hip, hydraulics.py: HydraulicNetwork.sensitivity, localize_leaks, sensitivity_ref, leak_scores_ref).
 * gatres_hydraulic_sensitivity takes the arguments of gatres_hydraulic_solve_links unchanged and in the same order, runs the same
 * loop (hy_newton<true>) on the same capped grid, one workgroup per scenario, and writes the same pressure, head, flow, status,
 * final_dq and link_state, bit for bit; here each of them may be NULL.  Then, in the same workgroup, for the K sensors
 * sensor_node int32[K] (nodes; duplicates are legal and give rows that are equal in every bit):
 * THE MATRIX.  The global-gradient matrix A of THE SOLVER (A_ii = sum 1/g_p, A_ij = -1/g_p over the junctions, unit rows for
 * the fixed-head nodes) is the Schur complement of the full Jacobian of (energy, mass) in (q, H), so dH/dd = -A^-1 for an outflow
 * d at a junction.  The kernel evaluates THE LINK LAW's g at the RETURNED flows (floor 1e-7 and 1e8 branches included: the
 * sensitivity is that of the kernel's own model), assembles A in the order of THE SOLVER's assembly, factorises it with the same
 * banded LDL^T, and solves the K unit right-hand sides at the sensors' solver rows against the resident factor, Kc at a time: all
 * right-hand sides of a chunk move together through each column step, the (band offset, right-hand side) pairs being the work
 * items, one barrier per column, the block [N][Kc] in LDS with the right-hand side's index fastest; each right-hand side takes
 * the operations of the loop's single vector in the same order, so a row does not depend on the chunk it falls in.
 * OUTPUTS, each optional (NULL: not wanted; what a launch computes is a compile-time fact of the instantiation it takes):
 *   dh_ddemand double[S][K][N]:  Z[k][n] = dH_sensor(k) / dd_n = -(A^-1)[row(k)][row(n)] in metres per m3/s, NEGATIVE where more
 *     outflow lowers the head; exactly +0.0 where n or the sensor is a fixed-head node.
 *   dh_droughness double[S][K][P]:  dH_sensor(k) / dC_p.  At fixed demands dH_a - dH_b = g_p dq_p + h_C dC_p, so a change of C_p
 *     moves the link's flow by -(h_C / g_p) dC_p at fixed heads: an outflow of that size at a and an inflow at b.  Hence
 *     (Z[k][a] - Z[k][b]) * (-h_C / g_p) with a -> b the link's direction, h_C = dh/dC = -1.852 r |q|^0.852 q / C, formed as
 *     ((1.852 * ra) * q) / (C * g_p), ra = r * pow(|q|, 0.852).  0 for a pump, for a link on a 1e8 branch (shut, or a CHECK link
 *     with q < 0) and for a pipe on the low-flow floor.  Raising C on a pipe that feeds the sensor raises its head.
 *   LOCALISATION, fused (no [S][K][N] in memory): readings double[S][K] are measured pressures in metres at the sensors, NaN
 *     where a sensor is missing in that scenario.  residual double[S][K]: rho_k = reading_k - (H_sensor(k) - elevation), in
 *     fp64 (not against the fp32 pressure), NaN where missing.  With z_n the column n of Z over the available sensors,
 *     leak_flow[s][n] = <z_n, rho> / <z_n, z_n>  (m3/s: the least-squares outflow at n alone) and
 *     score[s][n] = <z_n, rho> / (sqrt(<z_n, z_n>) * sqrt(<rho, rho>))  (the cosine; +1 is a perfect match for a leak at n),
 *     every sum over k ascending in fp64, product and sum rounded on their own, accumulated across chunks in LDS.  Both are NaN
 *     where n is a fixed-head node or <z_n, z_n> == 0.  If <rho, rho> == 0 or no sensor is available every score is NaN.
 *     best int32[S]: THE TIE RULE -- the lowest node index among those holding the maximum of the scores the kernel itself
 *     wrote (NaN scores take no part); -1 where every score is NaN.  Columns of junctions behind the same sensor cut are
 *     proportional, their scores differ by rounding alone: best names one of them, not the leak.
 * A scenario that ran out of iterations has its sensitivities computed from the returned flows (status tells it apart).  A
 * scenario that FAILED (status[s][2], or a bad pivot of the second factorisation, which does not touch status) has NaN in every
 * double output and best = -1.  A sensor_node outside [0, N) fails every scenario of the launch, as a bad static array does.
 * chunk: 0 takes Kc = the most right-hand sides that fit; a value > 0 caps Kc (no output depends on it).
 * NOT HERE: regulating valves (an ACTIVE valve's flow is lagged outside the matrix, so A is not the Jacobian), emitters as
 * unknowns and pressure-driven demand.
 * LDS need (hydraulics.sensitivity_lds_bytes, sensitivity_chunk): the bytes of gatres_hydraulic_solve_links
 *   + 16 N (the two score accumulators per row)  +  8 Kc (N + 1) (per right-hand side of a chunk its column and its residual),
 * Kc = min(K, (GATRES_HYD_LDS_BUDGET - links bytes - 16 N) / (8 (N + 1))), refused where Kc < 1.  On 388 nodes, 430 links, W = 19
 * without pumps: 92 264 + 6 208 bytes, Kc = 21.
 * GATRES_E_BADARG before any launch: what gatres_hydraulic_solve_links refuses (but for its NULL outputs); num_sensors < 1;
 * chunk < 0; sensor_node NULL; byte counts that do not fit; Kc < 1; readings given with none of residual, leak_flow, score and
 * best, or one of those without readings; an output overlapping an input or another output. */
int gatres_hydraulic_sensitivity(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                 const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                 int32_t half_bandwidth, const double* demand, const double* roughness, const double* fixed_head,
                                 int64_t fixed_head_stride, int64_t num_scenarios, int32_t num_nodes, int32_t num_pipes,
                                 double accuracy, int32_t max_iter, float* pressure, double* head, double* flow, int32_t* status,
                                 double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags, const double* minor,
                                 const int32_t* pump_link, const double* pump_h0, const double* pump_r, const double* pump_n,
                                 int32_t num_pumps, const double* speed, int64_t speed_stride, const uint8_t* closed,
                                 int64_t closed_stride, uint8_t* link_state, const int32_t* sensor_node, int32_t num_sensors,
                                 int32_t chunk, const double* readings, double* dh_ddemand, double* dh_droughness,
                                 double* residual, double* leak_flow, double* score, int32_t* best, void* stream);

const char* gatres_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GATRES_H */
