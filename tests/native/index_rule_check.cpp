// index_rule_check.cpp -- csrc/index_rule.h as a stand-alone host program (tests/test_index_cpu.py builds it plain and under the
// address / undefined-behaviour sanitizers and compares its output, line by line, with tests/index_ref.py on the same inputs).
// stdin, one request per line:
//   ppm dot nq n2                      -> the similarity in parts per million, and crosscam_rule.h's per mille beside it
//   slot rid capacity                  -> the slot of the row
//   slotrid slot capacity next_rid     -> the rid the slot holds (0 empty)
//   chunk capacity requested           -> the rows of a chunk (0: not allowed)
//   rank ppm rid                       -> the rank, then its ppm and rid taken apart again
//   search dim n nq k                  -> followed by n rows "rid dead t stream cls key v[dim]" and nq queries
//                                         "t0 t1 mask cls exclude_key min_ppm v[dim]"; per query one line "n_hits rid:ppm ..."
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "index_rule.h"

using namespace rtmodt;

int main() {
    std::string op;
    while (std::cin >> op) {
        if (op == "ppm") {
            long long dot, nq, n2;
            std::cin >> dot >> nq >> n2;
            std::printf("%d %d\n", ix_ppm((int32_t)dot, nq, n2), cc_sim((int32_t)dot, nq, n2));
        } else if (op == "slot") {
            long long rid, cap;
            std::cin >> rid >> cap;
            std::printf("%lld\n", (long long)ix_slot(rid, cap));
        } else if (op == "slotrid") {
            long long slot, cap, next;
            std::cin >> slot >> cap >> next;
            std::printf("%lld\n", (long long)ix_slot_rid(slot, cap, next));
        } else if (op == "chunk") {
            int cap, req;
            std::cin >> cap >> req;
            std::printf("%d\n", ix_chunk_rows(cap, req));
        } else if (op == "rank") {
            long long ppm, rid;
            std::cin >> ppm >> rid;
            const uint64_t r = ix_rank((int32_t)ppm, rid);
            std::printf("%llu %d %lld\n", (unsigned long long)r, ix_rank_ppm(r), (long long)ix_rank_rid(r));
        } else if (op == "search") {
            int dim, n, nq, k;
            std::cin >> dim >> n >> nq >> k;
            if (dim < 1 || dim > CC_MAX_DIM || n < 0 || nq < 0 || k < 1 || k > IX_MAX_K) return 2;
            std::vector<long long> rid(n), t(n), key(n), n2(n);
            std::vector<int> dead(n), stream(n), cls(n);
            std::vector<int8_t> rows((size_t)n * dim);
            for (int i = 0; i < n; ++i) {
                std::cin >> rid[i] >> dead[i] >> t[i] >> stream[i] >> cls[i] >> key[i];
                for (int d = 0; d < dim; ++d) { int v; std::cin >> v; rows[(size_t)i * dim + d] = (int8_t)v; n2[i] += v * v; }
            }
            for (int q = 0; q < nq; ++q) {
                long long t0, t1, excl; unsigned long long mask; int cq, min_ppm;
                std::cin >> t0 >> t1 >> mask >> cq >> excl >> min_ppm;
                std::vector<int> v(dim);
                long long nqq = 0;
                for (int d = 0; d < dim; ++d) { std::cin >> v[d]; nqq += v[d] * v[d]; }
                uint64_t best[IX_MAX_K];
                int nb = 0;
                for (int i = 0; i < n; ++i) {
                    if (!ix_row_ok(rid[i], dead[i], t[i], stream[i], cls[i], key[i], t0, t1, mask, cq, excl)) continue;
                    int32_t dot = 0;
                    for (int d = 0; d < dim; ++d) dot += v[d] * rows[(size_t)i * dim + d];
                    const int32_t ppm = ix_ppm(dot, nqq, n2[i]);
                    if (ppm >= min_ppm) ix_topk_insert(best, nb, k, ix_rank(ppm, rid[i]));
                }
                std::printf("%d", nb);
                for (int i = 0; i < nb; ++i) std::printf(" %lld:%d", (long long)ix_rank_rid(best[i]), ix_rank_ppm(best[i]));
                std::printf("\n");
            }
        } else {
            return 3;
        }
    }
    return 0;
}
