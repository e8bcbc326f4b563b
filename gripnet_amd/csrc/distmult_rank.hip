// Filtered ranking and top-k partner retrieval for the DistMult decoder (link-prediction evaluation).
//
// A query is a row (u, r); its candidate scores are the logits s(v) = sum_k z[u,k] D[r,k] z[v,k] for every v in [0, n):
// one row of the skinny product (z[u] * D[r]) @ z^T, K = num_features.  One score engine, two epilogues:
//   rank  (gn_distmult_rank_f32): per query (u, r, v_true) the counts of the non-known candidates v != v_true with
//         s(v) > s(v_true) and s(v) == s(v_true);
//   top-k (gn_distmult_topk_f32): per query (u, r) the k <= 64 best non-known candidates, score descending then id ascending.
// Nothing of the [Q, n] score matrix reaches memory.
//
// Engine.  A workgroup is four waves; a wave owns 16 query rows (the M of v_mfma_f32_16x16x4_f32, an exact fp32 FMA chain
// on gfx950).  Its A operand, z[u] * D[r] per row (rows of different relations share a tile), is formed on load and kept in
// registers for the whole scan: lane l holds features kq * S + s (kq = l >> 4, s < S) of row l & 15, the features padded
// with zeros to 4 S (a multiple of 16).  z streams through LDS as B, 64 columns (four 16-column MFMA tiles) per stage,
// shared by the four waves; every wave runs two tiles' chains interleaved.  Output element (row 4 (l >> 4) + j, column
// l & 15) sits in register j of lane l.
//
// The true score.  An MFMA output element depends only on its A row, its B column and the order of the K steps, so the
// rank kernel computes s(v_true) in a prologue tile whose B column j is z[v_true] of the wave's query j (the same floats
// the stage holds for that column), through the same chain: the diagonal of that tile is bit-identical to what the scan
// computes at column v_true.  A pair recomputed in another order could count itself as a near-tie or a "greater".
//
// Filter.  gn_known_pairs (negsample.hip) keeps one sorted partner row per (r, u).  Per window of 2,048 columns every wave
// sets the bits of its 16 rows' partners in a [16][64]-word LDS bitmap (LDS integer OR: the same bits whatever the order);
// the epilogue tests one bit per output element.
//
// Top-k.  Per row the wave keeps a list of up to k entries (sorted) and a buffer of kCap candidates in LDS, and in
// registers the list's last entry as a threshold.  An element that beats the threshold is appended (slot from a ballot
// prefix: no atomics, the same slots every run); before a buffer can overflow, list and buffer are merged by rank counting
// (the order is total: ids are unique), which is deterministic as well.
//
// Candidate ranges (the _ranged entry points).  A table [R][2] of (lo, hi) per relation admits candidate v for a query of
// relation r iff lo_r <= v < hi_r, on top of the rules above: a query reads its row once, the workgroup scans the stages
// that hold a column of the union of its valid queries' ranges (rounded down to a stage; the first bitmap window is built
// from its own start) and masks per row.  A score does not depend on where the scan starts, so a ranged result is the
// full scan's restricted to the range, bit for bit; without a table every range is (0, n).
//
// The engine itself is rank_engine.cuh: kge_rank.hip runs it as well, with prepared query rows as the A operand.
#include "rank_engine.cuh"

extern "C" {

gn_status gn_distmult_rank_ranged_f32(const float* z, int64_t ld_z, int64_t n, int64_t f, const float* d, int64_t ld_d, int64_t R,
                                      const int64_t* u, const int64_t* v, const int64_t* et, int64_t Q, const gn_known_pairs* known,
                                      int32_t* greater, int32_t* ties, int32_t* err, void* stream, const int64_t* cand_range) {
    RankArgs a;
    int S = 0;
    const gn_status s = fill_args(a, z, ld_z, n, f, d, ld_d, R, u, et, Q, known, cand_range, err, S);
    if (s != GN_OK) return s;
    if (Q == 0) return GN_OK;
    GN_REQUIRE(z && d && u && v && et && greater && ties, "operand pointer is null");
    GN_REQUIRE(n > 0 && R > 0, "queries given but the node or relation table is empty");
    a.v = v; a.greater = greater; a.ties = ties;
    return launch<false>(a, S, gn::as_stream(stream));
}

gn_status gn_distmult_rank_f32(const float* z, int64_t ld_z, int64_t n, int64_t f, const float* d, int64_t ld_d, int64_t R,
                               const int64_t* u, const int64_t* v, const int64_t* et, int64_t Q, const gn_known_pairs* known,
                               int32_t* greater, int32_t* ties, int32_t* err, void* stream) {
    return gn_distmult_rank_ranged_f32(z, ld_z, n, f, d, ld_d, R, u, v, et, Q, known, greater, ties, err, stream, nullptr);
}

gn_status gn_distmult_topk_ranged_f32(const float* z, int64_t ld_z, int64_t n, int64_t f, const float* d, int64_t ld_d, int64_t R,
                                      const int64_t* u, const int64_t* et, int64_t Q, int64_t k, const gn_known_pairs* known,
                                      float* scores, int64_t* ids, int32_t* err, void* stream, const int64_t* cand_range) {
    GN_REQUIRE(k >= 1 && k <= kMaxK, "k must be in [1, %d], got %lld", kMaxK, (long long)k);
    RankArgs a;
    int S = 0;
    const gn_status s = fill_args(a, z, ld_z, n, f, d, ld_d, R, u, et, Q, known, cand_range, err, S);
    if (s != GN_OK) return s;
    if (Q == 0) return GN_OK;
    GN_REQUIRE(z && d && u && et && scores && ids, "operand pointer is null");
    GN_REQUIRE(n > 0 && R > 0, "queries given but the node or relation table is empty");
    a.scores = scores; a.ids = ids; a.k = (int)k;
    return launch<true>(a, S, gn::as_stream(stream));
}

gn_status gn_distmult_topk_f32(const float* z, int64_t ld_z, int64_t n, int64_t f, const float* d, int64_t ld_d, int64_t R,
                               const int64_t* u, const int64_t* et, int64_t Q, int64_t k, const gn_known_pairs* known,
                               float* scores, int64_t* ids, int32_t* err, void* stream) {
    return gn_distmult_topk_ranged_f32(z, ld_z, n, f, d, ld_d, R, u, et, Q, k, known, scores, ids, err, stream, nullptr);
}

}  // extern "C"
