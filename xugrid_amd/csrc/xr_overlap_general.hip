// xr_overlap_general.hip -- the general kernel chain of the weight construction (overlap_general): any pair of meshes, polygon
// meshes included, and the fall-back of the fused pipeline.  search -> [host: C] -> clip (+ row counts by global atomics) ->
// scan -> [host: nnz] -> row_fill, all on the engine stream; the stages are described at the head of xr_overlap.hip, which
// also holds the kernels this chain shares with the fused pipeline (k_search, k_search_big, k_row_fill_long).
#include "xr_overlap.h"
#include "xr_clip.h"

namespace xr {

// The chain keeps four device words and uses four mailbox slots of its own.
enum GenWord : int {
    GEN_CLIP_OVERFLOW = 0, // pairs whose clipped polygon did not fit the small buffer (redone with the oracle's size)
    GEN_N_PENDING = 1,     // big faces that did not fit the queue; k_publish hands it to the host and zeroes it ...
    GEN_N_LONG_ROWS = 1,   // ... so that the same word then counts the rows k_row_fill leaves to k_row_fill_long
    GEN_N_BIG = 2,         // big faces (k_search)
    GEN_QUEUE_CURSOR = 3,  // pairs in the queue
    GEN_WORDS = 4
};
enum GenMailSlot : int { GMAIL_PAIRS = 0, GMAIL_NNZ = 1, GMAIL_CLIP_OVERFLOW = 2, GMAIL_N_PENDING = 3 };

// deposit one device word in the host mailbox (pinned memory)
__global__ void k_publish(const int32_t *__restrict__ src, int32_t *dst, int32_t *src2, int32_t *dst2) {
    if (threadIdx.x == 0) {
        *dst = *src;
        *dst2 = *src2;
        *src2 = 0; // the counter is reused afterwards
    }
}

template <int MAXV, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
k_clip(const double *__restrict__ q_fxy, const uint8_t *__restrict__ q_len, const int32_t *__restrict__ q_off, int q_m,
       const int32_t *__restrict__ q_perm, const double *__restrict__ s_fxy, const uint8_t *__restrict__ s_len, const int32_t *__restrict__ s_off,
       int s_m, const int32_t *__restrict__ cand_tgt, const int32_t *__restrict__ cand_src, int64_t n_cand,
       double *__restrict__ cand_area, bool redo_only, const int32_t *__restrict__ rec_face,
       int32_t *__restrict__ cand_sid, int32_t *__restrict__ overflow_count, int32_t *__restrict__ nnz_row, double dust) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2 *sh = reinterpret_cast<double2 *>(smem);
    const int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool active = c < n_cand && !(redo_only && cand_area[c] != AREA_OVERFLOW);
    int t = -1, nt = 0, ns = 0;
    const double2 *tf = nullptr;
    const double *sf = nullptr;
    double area = 0.0;
    if (active) {
    t = cand_tgt[c];
    const int s = cand_src[c];
    cand_sid[c] = rec_face[s];
    nt = q_len[t], ns = s_len[s];
    double2 *out = sh + threadIdx.x;                // out[j * BLOCK]
    double2 *in = sh + MAXV * BLOCK + threadIdx.x;  // in[j * BLOCK]
    tf = reinterpret_cast<const double2 *>(q_fxy) + face_vertex_base(q_off, t, q_m);
    sf = s_fxy + 2 * face_vertex_base(s_off, s, s_m);
    for (int j = 0; j < nt; j++) out[j * BLOCK] = tf[j];
    int n_output = nt;
    bool overflow = false;
    P2 r = load_p2(sf, ns - 1);
    bool empty = false;
    for (int i = 0; i < ns; i++) {
        const P2 sv = load_p2(sf, i);
        const P2 U{sv.x - r.x, sv.y - r.y};
        if (U.x == 0 && U.y == 0) continue;
        const P2 N{-U.y, U.x};
        const int length = n_output;
        {
            double2 *tmp = in;
            in = out;
            out = tmp;
        }
        n_output = 0;
        const double2 a2 = in[(length - 1) * BLOCK];
        P2 a{a2.x, a2.y};
        bool a_inside = sh_inside(a, r, U);
        for (int j = 0; j < length; j++) {
            const double2 b2 = in[j * BLOCK];
            const P2 b{b2.x, b2.y};
            const P2 V{b.x - a.x, b.y - a.y};
            if (V.x == 0 && V.y == 0) continue;
            bool b_inside = sh_inside(b, r, U);
            if (b_inside) {
                if (!a_inside) {
                    P2 pt;
                    if (sh_intersection(a, V, r, N, pt)) {
                        if (n_output < MAXV) out[n_output * BLOCK] = make_double2(pt.x, pt.y);
                        else overflow = true;
                        n_output++;
                    }
                }
                if (n_output < MAXV) out[n_output * BLOCK] = b2;
                else overflow = true;
                n_output++;
            } else if (a_inside) {
                P2 pt;
                if (sh_intersection(a, V, r, N, pt)) {
                    if (n_output < MAXV) out[n_output * BLOCK] = make_double2(pt.x, pt.y);
                    else overflow = true;
                    n_output++;
                } else {
                    b_inside = true;
                    if (n_output < MAXV) out[n_output * BLOCK] = b2;
                    else overflow = true;
                    n_output++;
                }
            }
            a = b;
            a_inside = b_inside;
        }
        if (overflow) break;
        if (n_output < 3) {
            empty = true;
            break;
        }
        r = sv;
    }
    if (overflow) {
        area = AREA_OVERFLOW;
    } else if (!empty) {
        // fan area from the first clipped vertex (local origin)
        const double2 a2 = out[0];
        const double2 b2 = out[BLOCK];
        double ux = b2.x - a2.x, uy = b2.y - a2.y;
        for (int i = 2; i < n_output; i++) {
            const double2 c2 = out[i * BLOCK];
            const double vx = a2.x - c2.x, vy = a2.y - c2.y;
            area += fabs(ux * vy - uy * vx);
            ux = vx;
            uy = vy;
        }
        area = 0.5 * area;
    }
    } // active
    clip_epilogue(area, dust, active, c, t, tf, nt, reinterpret_cast<const double2 *>(sf), ns, cand_area, overflow_count, nnz_row);
}

template <int MAXV, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
k_clip_small(const double *__restrict__ q_fxy, const uint8_t *__restrict__ q_len, const int32_t *__restrict__ q_off, int q_m,
             const int32_t *__restrict__ q_perm, const double *__restrict__ s_fxy,
             const uint8_t *__restrict__ s_len, const int32_t *__restrict__ s_off, int s_m, const int32_t *__restrict__ cand_tgt,
             const int32_t *__restrict__ cand_src, int64_t n_cand, double *__restrict__ cand_area,
             const int32_t *__restrict__ rec_face, int32_t *__restrict__ cand_sid,
             int32_t *__restrict__ overflow_count, int32_t *__restrict__ nnz_row, bool remap, double dust) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2 *out = reinterpret_cast<double2 *>(smem) + threadIdx.x; // out[j * BLOCK]
    const int64_t n_blocks = (n_cand + BLOCK - 1) / BLOCK;
    const int64_t lb = xcd_block(n_blocks, remap);
    if (lb >= n_blocks) return;
    const int64_t c = lb * BLOCK + threadIdx.x;
    const bool active = c < n_cand;
    int t = -1, nt = 0, ns = 0;
    const double2 *tf = nullptr;
    const double *sf = nullptr;
    double area = 0.0;
    if (active) {
        t = cand_tgt[c];
        const int s = cand_src[c];
        cand_sid[c] = rec_face[s];
        nt = q_len[t], ns = s_len[s];
        tf = reinterpret_cast<const double2 *>(q_fxy) + face_vertex_base(q_off, t, q_m);
        sf = s_fxy + 2 * face_vertex_base(s_off, s, s_m);
        area = clip_small_pair<MAXV, BLOCK>(tf, nt, sf, ns, out);
    }
    clip_epilogue(area, dust, active, c, t, tf, nt, reinterpret_cast<const double2 *>(sf), ns, cand_area, overflow_count, nnz_row);
}

// A triangle source against targets of N0 = 3 or 4 vertices: the flag / compaction formulation of xr_clip_tri.h -- about half the
// instructions of k_clip_small, same areas bit for bit.  N0 = 3: both meshes are pure triangle meshes.  N0 = 4: quadrilateral
// (raster / quad mesh) targets -- the shape of the reference's unstructured -> raster regridding -- whose faces may be triangles
// with a fill slot (q_len, read for N0 = 4 only); replaces k_clip_small<8> for this pair of shapes.
template <int BLOCK, int N0>
__global__ void __launch_bounds__(BLOCK)
k_clip_tri(const double *__restrict__ q_fxy, const uint8_t *__restrict__ q_len, const double *__restrict__ s_fxy,
           const int32_t *__restrict__ cand_tgt, const int32_t *__restrict__ cand_src, int64_t n_cand,
           double *__restrict__ cand_area, const int32_t *__restrict__ rec_face, int32_t *__restrict__ cand_sid,
           int32_t *__restrict__ overflow_count, int32_t *__restrict__ nnz_row, bool remap, double dust) {
    static_assert(N0 == 3 || N0 == 4, "triangle or quadrilateral subject");
    constexpr int MAXV = N0 == 3 ? TRI_MAXV : QUAD_MAXV;
    // slots per lane: TRI_MAXV + 1, 112 bytes; QUAD_MAXV + 2, 144 bytes -- 128 would put the 16-byte accesses of all lanes on the
    // same banks
    constexpr int COL = N0 == 3 ? TRI_MAXV + 1 : QUAD_MAXV + 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2 *col = reinterpret_cast<double2 *>(smem) + threadIdx.x * COL;
    __shared__ uint2 sh_lut[N0 == 3 ? TRI_LUT : QUAD_LUT];
    const int64_t n_blocks = (n_cand + BLOCK - 1) / BLOCK;
    const int64_t lb = xcd_block(n_blocks, remap);
    if (lb >= n_blocks) return;
    poly_lut_init<MAXV>(sh_lut);
    __syncthreads();
    const int64_t c = lb * BLOCK + threadIdx.x;
    const bool active = c < n_cand;
    int t = -1, n0 = 3, s = 0;
    P2 tv[N0] = {}, sv[3] = {};
    if (active) {
        t = cand_tgt[c];
        s = cand_src[c];
        cand_sid[c] = rec_face[s];
        if (N0 > 3) n0 = q_len[t];
    }
    const double2 *tf = reinterpret_cast<const double2 *>(q_fxy) + (int64_t)t * N0;
    const double2 *sf = reinterpret_cast<const double2 *>(s_fxy) + (int64_t)s * 3;
    if (active) {
#pragma unroll
        for (int j = 0; j < N0; j++) {
            if (j < n0) {
                const double2 a = tf[j];
                tv[j] = P2{a.x, a.y};
            }
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double2 b = sf[j];
            sv[j] = P2{b.x, b.y};
        }
    }
    const double area = poly_clip_area<MAXV, N0>(tv, n0, sv, col, sh_lut, active);
    clip_epilogue(area, dust, active, c, t, tf, n0, sf, 3, cand_area, overflow_count, nnz_row);
}

// ---------------------------------------------------------------------------------------------
// CSR assembly
// ---------------------------------------------------------------------------------------------
// recount of the survivors per row; only used after the rare clip-buffer overflow redo
__global__ void __launch_bounds__(256) k_row_count(const int32_t *__restrict__ cand_off,
                                                  const int32_t *__restrict__ cand_count,
                                                  const double *__restrict__ cand_area, int64_t n_query,
                                                  const int32_t *__restrict__ q_perm,
                                                  int32_t *__restrict__ nnz_row) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_query) return;
    int n = 0;
    for (int c = cand_off[t]; c < cand_off[t] + cand_count[t]; c++) n += cand_area[c] > 0 ? 1 : 0;
    nnz_row[t] = n;
}

static constexpr int ROW_SHORT = 24; // rows with more candidates go to the block-per-row kernel

static constexpr int ROW_LDS = 3072; // short-row candidate entries one block can stage in LDS

// One block = 256 consecutive query faces (query order).  The candidate entries of the block's
// SHORT rows (<= ROW_SHORT candidates; long rows go to k_row_fill_long) are packed into LDS -- the
// block's candidate segment is contiguous, so the loads are coalesced -- then the block works
// ENTRY-parallel: each thread takes entries, ranks a survivor among the survivors of its row
// (adjacent in LDS) and writes it to its final CSR position.  Rows are stored in QUERY order
// (row r belongs to the caller's face q_perm[r], xr_csr::stored.row_order).
__global__ void __launch_bounds__(256)
k_row_fill(const int32_t *__restrict__ cand_off, const int32_t *__restrict__ cand_count,
           const int2 *__restrict__ block_seg, const uint8_t *__restrict__ is_big,
           const int32_t *__restrict__ cand_tgt, const int32_t *__restrict__ cand_sid,
           const double *__restrict__ cand_area, int64_t n_query,
           const int32_t *__restrict__ indptr, const double *__restrict__ src_area, bool relative,
           int32_t *__restrict__ indices, double *__restrict__ data, int32_t *__restrict__ long_rows,
           int32_t *__restrict__ n_long, int32_t *__restrict__ apply_long_rows,
           int32_t *__restrict__ n_apply_long, bool remap) {
    __shared__ int32_t sh_src[ROW_LDS];  // tree face id of a survivor, INT_MAX for area <= 0
    __shared__ uint16_t sh_row[ROW_LDS];
    __shared__ int32_t sh_c0[256];   // first candidate of the row (global index)
    __shared__ int32_t sh_lds[257];  // LDS offset of the row (short rows only), [256] = total
    __shared__ int32_t sh_ptr[256];  // CSR offset of the row
    __shared__ int32_t sh_wave[4];
    const int64_t n_blocks = (n_query + 255) / 256;
    const int64_t lb = xcd_block(n_blocks, remap);
    if (lb >= n_blocks) return;
    const int64_t t0 = lb * 256;
    const int64_t t = t0 + threadIdx.x;
    // the candidates of the block's rows that k_search wrote itself (all but its "big" faces) are one stretch
    const int2 seg = block_seg[lb];
    const int seg0 = seg.x, seg1 = seg.x + seg.y;
    int c0 = 0, len = 0;
    bool is_short = true; // packed here; everything else (long rows, and the "big" faces of the search, whose
                          // candidates live elsewhere in the queue) goes to the block-per-row kernel
    if (t < n_query) {
        c0 = cand_off[t];
        len = cand_count[t];
        is_short = len <= ROW_SHORT && !is_big[t];
        sh_ptr[threadIdx.x] = indptr[t];
        if (!is_short) long_rows[atomicAdd(n_long, 1)] = (int32_t)t;
        if (indptr[t + 1] - indptr[t] > XR_APPLY_LONG_ROW) apply_long_rows[atomicAdd(n_apply_long, 1)] = (int32_t)t;
    }
    const int slen = is_short ? len : 0;
    sh_c0[threadIdx.x] = is_short ? c0 : -1;
    // block exclusive scan of the short-row lengths
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan(slen);
    if (lane == 63) sh_wave[wave] = incl;
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < wave) woff += sh_wave[w];
        total += sh_wave[w];
    }
    sh_lds[threadIdx.x] = woff + incl - slen;
    if (threadIdx.x == 0) sh_lds[256] = total;
    __syncthreads();
    if (total <= ROW_LDS) {
        for (int j = seg0 + threadIdx.x; j < seg1; j += 256) {
            const int row = cand_tgt[j] - (int)t0;
            const int rc0 = sh_c0[row];
            if (rc0 < 0) continue; // entry of a long row
            const int k = sh_lds[row] + (j - rc0);
            sh_src[k] = cand_area[j] > 0 ? cand_sid[j] : 0x7fffffff;
            sh_row[k] = (uint16_t)row;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < total; k += 256) {
            const int s = sh_src[k];
            if (s == 0x7fffffff) continue;
            const int row = sh_row[k];
            const int a0 = sh_lds[row], a1 = row == 255 ? total : sh_lds[row + 1];
            int rank = 0;
            for (int i = a0; i < a1; i++) rank += sh_src[i] < s ? 1 : 0;
            const double a = cand_area[sh_c0[row] + (k - a0)];
            const int pos = sh_ptr[row] + rank;
            indices[pos] = s;
            data[pos] = relative ? a / src_area[s] : a;
        }
    } else if (t < n_query && is_short) {
        // more short-row candidates than the LDS stage holds: rank straight from memory
        const int base = indptr[t];
        for (int i = c0; i < c0 + len; i++) {
            const double a = cand_area[i];
            if (!(a > 0)) continue;
            const int s = cand_sid[i];
            int rank = 0;
            for (int j = c0; j < c0 + len; j++) rank += (cand_area[j] > 0 && cand_sid[j] < s) ? 1 : 0;
            indices[base + rank] = s;
            data[base + rank] = relative ? a / src_area[s] : a;
        }
    }
}

template <int MAXV, int BLOCK>
static void launch_clip(const xr_mesh *tree, const xr_mesh *query, const int32_t *cand_tgt, const int32_t *cand_src,
                        int64_t C, double *cand_area, bool redo_only, int32_t *cand_sid, int32_t *overflow_count,
                        int32_t *nnz_row) {
    constexpr size_t shmem = (size_t)2 * MAXV * BLOCK * sizeof(double2);
    allow_dynamic_lds<&k_clip<MAXV, BLOCK>>(shmem);
    XR_LAUNCH(MAXV == 8 ? "clip_v8" : (MAXV == 16 ? "clip_v16" : "clip_v64"), (k_clip<MAXV, BLOCK>),
              dim3(div_up(C, BLOCK)), dim3(BLOCK), shmem, query->qo_fxy(), query->qo_len(), query->qo_off(), query->m,
              query->qo_perm(), tree->index.rec_fxy.get(), tree->index.rec_len.get(), tree->record_off(), tree->m, cand_tgt, cand_src, C, cand_area,
              redo_only, tree->index.rec_face.get(), cand_sid, overflow_count, nnz_row, overlap_dust_threshold(tree, query));
}

static void launch_clip_for(const xr_mesh *tree, const xr_mesh *query, const int32_t *cand_tgt, const int32_t *cand_src,
                            int64_t C, double *cand_area, int32_t *cand_sid, int32_t *overflow_count,
                            int32_t *nnz_row) {
    const int vmax = query->m + tree->m;
    if (vmax > 16) return launch_clip<64, 64>(tree, query, cand_tgt, cand_src, C, cand_area, false, cand_sid, overflow_count, nnz_row);
    if (vmax > 8) return launch_clip<16, 128>(tree, query, cand_tgt, cand_src, C, cand_area, false, cand_sid, overflow_count, nnz_row);
    constexpr int BLOCK = 256;
    const bool remap = REMAP_CLIP;
    const dim3 grid(xcd_grid(div_up(C, BLOCK), remap));
    const double dust = overlap_dust_threshold(tree, query);
    if (vmax <= 6) {
        // triangle x triangle: the clipped polygon never has more than 6 vertices
        constexpr int MAXV = 6;
        const size_t shmem = (size_t)(MAXV + 1) * BLOCK * sizeof(double2); // + one trash row for clamped pushes
        XR_LAUNCH("clip_tri", (k_clip_tri<BLOCK, 3>), grid, dim3(BLOCK), shmem, query->qo_fxy(), (const uint8_t *)nullptr,
                  tree->index.rec_fxy.get(), cand_tgt, cand_src, C, cand_area, tree->index.rec_face.get(), cand_sid, overflow_count, nnz_row, remap,
                  dust);
    } else if (query->m == 4 && tree->m == 3 && option(OPT_CLIP_QUAD) != 0) {
        // quadrilateral targets (a raster) x triangle source (option "clip_quad" = 0: the slot-loop kernel, test switch)
        const size_t shmem = (size_t)(QUAD_MAXV + 2) * BLOCK * sizeof(double2);
        XR_LAUNCH("clip_quad_tri", (k_clip_tri<BLOCK, 4>), grid, dim3(BLOCK), shmem,
                  query->qo_fxy(), query->qo_len(), tree->index.rec_fxy.get(), cand_tgt, cand_src, C, cand_area, tree->index.rec_face.get(),
                  cand_sid, overflow_count, nnz_row, remap, dust);
    } else {
        constexpr int MAXV = 8;
        const size_t shmem = (size_t)(MAXV + 1) * BLOCK * sizeof(double2); // + one trash row for clamped pushes
        XR_LAUNCH("clip_small", (k_clip_small<MAXV, BLOCK>), grid, dim3(BLOCK),
                  shmem, query->qo_fxy(), query->qo_len(), query->qo_off(), query->m, query->qo_perm(), tree->index.rec_fxy.get(),
                  tree->index.rec_len.get(), tree->record_off(), tree->m, cand_tgt, cand_src, C, cand_area, tree->index.rec_face.get(), cand_sid,
                  overflow_count, nnz_row, remap, dust);
    }
}

// The general kernel chain, all on the engine stream: two host round trips, rows in query order.
void overlap_general(xr_mesh *tree, xr_mesh *query, const double *tree_area, bool relative, xr_csr *csr, const MortonParams &tile) {
    const int64_t T = query->n_face;
    hipStream_t st = launch_stream();
    DevBuf<int32_t> counters(GEN_WORDS); // (GenWord)
    auto word = [&](GenWord w) { return counters.get() + w; };
    XR_HIP(hipMemsetAsync(counters.get(), 0, sizeof(int32_t) * GEN_WORDS, st));
    // --- candidate search.  k_search appends the candidates of its 256 faces to the pair queue itself (one
    // atomic reservation per block); the few "big" faces are counted, reserve their stretch, and are filled by
    // the block-per-face kernels.  The queue is sized for the regular faces (at most SLOTS candidates each) plus
    // a margin for the big ones; if the big faces need more, it is regrown before they are filled (rare).
    SearchLists l(T);
    const int64_t margin_opt = option(OPT_QUEUE_MARGIN); // test hook: a tiny margin forces the regrow path
    int64_t capacity = T * SLOTS + (margin_opt > 0 ? margin_opt : ((int64_t)4 << 20));
    XR_REQUIRE(capacity < ((int64_t)1 << 31), XR_ERR_LIMIT, "candidate pair queue exceeds the int32 range");
    DevBuf<int32_t> cand_tgt((size_t)capacity), cand_src((size_t)capacity);
    const PairQueue queue{cand_tgt.get(), cand_src.get(), word(GEN_QUEUE_CURSOR), capacity};
    launch_search(tree, query, l, queue, word(GEN_N_BIG), tile, csr->tiling.pending ? csr->tiling.key.get() : nullptr);
    launch_search_big(tree, query, l, queue, word(GEN_N_BIG), word(GEN_N_PENDING));
    // queue length and number of big faces still to be filled -> host
    int32_t *mail = const_cast<int32_t *>(engine().mailbox);
    XR_LAUNCH("publish", k_publish, dim3(1), dim3(64), 0, word(GEN_QUEUE_CURSOR), mail + GMAIL_PAIRS, word(GEN_N_PENDING),
              mail + GMAIL_N_PENDING);
    mailbox_wait();
    const int32_t C32 = mail[GMAIL_PAIRS], n_pending = mail[GMAIL_N_PENDING];
    XR_REQUIRE(C32 >= 0, XR_ERR_LIMIT, "candidate pair count exceeds the int32 range");
    const int64_t C = C32;
    tree->last_candidates = C;
    if (n_pending > 0) {
        // some big faces need more room than the margin: move what is there to a larger queue, then fill them
        DevBuf<int32_t> bigger_tgt((size_t)C), bigger_src((size_t)C);
        XR_HIP(hipMemcpyAsync(bigger_tgt.get(), cand_tgt.get(), sizeof(int32_t) * (size_t)capacity, hipMemcpyDeviceToDevice, st));
        XR_HIP(hipMemcpyAsync(bigger_src.get(), cand_src.get(), sizeof(int32_t) * (size_t)capacity, hipMemcpyDeviceToDevice, st));
        stream_sync();
        cand_tgt = std::move(bigger_tgt);
        cand_src = std::move(bigger_src);
        capacity = C;
        h2d(word(GEN_N_PENDING), &n_pending, sizeof(int32_t)); // (k_publish zeroed the device copy)
        launch_search_big_fill(tree, query, l, PairQueue{cand_tgt.get(), cand_src.get(), nullptr, capacity}, word(GEN_N_PENDING));
        XR_HIP(hipMemsetAsync(word(GEN_N_PENDING), 0, sizeof(int32_t), st));
    }
    // (the word of GEN_N_PENDING is zero again: from here on it is GEN_N_LONG_ROWS)
    DevBuf<int32_t> cand_sid((size_t)C);
    DevBuf<double> cand_area((size_t)C);
    if (C > 0) {
        // --- clip (+ per-row survivor counts)
        launch_clip_for(tree, query, cand_tgt.get(), cand_src.get(), C, cand_area.get(), cand_sid.get(), word(GEN_CLIP_OVERFLOW),
                        l.nnz_row.get());
    }
    // --- rows
    // P is needed on the host anyway; the overflow counter travels in the same mailbox round trip
    exclusive_scan_i32(l.nnz_row.get(), csr->indptr.get(), T, mail + GMAIL_NNZ, word(GEN_CLIP_OVERFLOW), mail + GMAIL_CLIP_OVERFLOW);
    mailbox_wait();
    int32_t nnz = mail[GMAIL_NNZ];
    if (mail[GMAIL_CLIP_OVERFLOW] > 0) {
        // polygon buffer overflow in the small-MAXV kernel (floating-point degenerate pairs):
        // redo those pairs with the oracle's buffer size, then recount every row.
        XR_HIP(hipMemsetAsync(word(GEN_CLIP_OVERFLOW), 0, sizeof(int32_t), st));
        XR_HIP(hipMemsetAsync(l.nnz_row.get(), 0, sizeof(int32_t) * (size_t)T, st));
        launch_clip<64, 64>(tree, query, cand_tgt.get(), cand_src.get(), C, cand_area.get(), true, cand_sid.get(),
                            word(GEN_CLIP_OVERFLOW), l.nnz_row.get());
        XR_LAUNCH("row_recount", k_row_count, dim3(div_up(T, 256)), dim3(256), 0, l.cand_off.get(), l.cand_count.get(),
                  cand_area.get(), T, query->qo_perm(), l.nnz_row.get());
        exclusive_scan_i32(l.nnz_row.get(), csr->indptr.get(), T);
        nnz = read_scalar(csr->indptr.get() + T);
    }
    XR_REQUIRE(nnz >= 0, XR_ERR_LIMIT, "nnz exceeds the int32 range");
    const int64_t P = nnz;
    csr->nnz = P;
    csr->indices.alloc((size_t)P);
    csr->data.alloc((size_t)P);
    // rows are best processed in the query mesh's spatial order (apply kernels)
    if (query->qo_perm()) {
        csr->stored.row_order.alloc((size_t)T);
        XR_HIP(hipMemcpyAsync(csr->stored.row_order.get(), query->qo_perm(), sizeof(int32_t) * (size_t)T,
                              hipMemcpyDeviceToDevice, st));
        csr->stored.has_row_order = true;
    }
    if (P > 0) {
        DevBuf<int32_t> long_rows((size_t)T);
        csr->longs.begin((size_t)(P / XR_APPLY_LONG_ROW + 1));
        csr->longs.end(1); // (not read back: the applies launch the long rows' kernels, which may find the list empty)
        const bool remap = REMAP_ROW_FILL;
        XR_LAUNCH("row_fill", k_row_fill, dim3(xcd_grid(div_up(T, 256), remap)), dim3(256), 0, l.cand_off.get(), l.cand_count.get(),
                  l.block_seg.get(), l.is_big.get(), cand_tgt.get(), cand_sid.get(), cand_area.get(), T, csr->indptr.get(), tree_area, relative,
                  csr->indices.get(), csr->data.get(), long_rows.get(), word(GEN_N_LONG_ROWS), csr->longs.rows.get(),
                  csr->longs.n_dev.get(), remap);
        launch_row_fill_long(0, tree, l, tree_area, relative,
                             LongRows{cand_sid.get(), cand_area.get(), csr->indptr.get(), csr->indices.get(), csr->data.get(),
                                      long_rows.get(), word(GEN_N_LONG_ROWS), -1});
    }
}

} // namespace xr
