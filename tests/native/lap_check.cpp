// Host-side check of the sparse assignment solver (csrc/lap.h: lap_solve) for its three cost types, compiled by
// tests/test_lap_cpu.py (once plain, once with the address and undefined-behaviour sanitizers).  Every LapSmemT array is a
// heap block of exactly its documented size (LAP_ROWS, LAP_COLS, LAP_EDGES, LAP_ROWS + 1), so an overrun is a heap overrun.
// Exit code 0 and one line "ok <family> <type> ..." per family and cost type on success; the first counter-example otherwise.
//
//   lap_check [problems.txt]      problems.txt: generic double problems written by the test; one "obj <i> <objective>" line each
//
// Gains are integers k in 1..1023; the edge cost of gain k is  double: -k/1024   LexCost: (-1, (1024-k)/1024)   long long: -k,
// so every sum and difference the solver forms is exact and the dual checks below need no tolerance.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "lap.h"
using namespace rtmodt;

template <typename C> struct Tr;
template <> struct Tr<double> {
    static const char *name() { return "double"; }
    static double make(int k) { return -(double)k / 1024.0; }
    static void print(double c) { printf("%.17g", c); }
};
template <> struct Tr<LexCost> {
    static const char *name() { return "LexCost"; }
    static LexCost make(int k) { return LexCost{-1, (double)(1024 - k) / 1024.0}; }
    static void print(LexCost c) { printf("(%d, %.17g)", c.n, c.d); }
};
template <> struct Tr<long long> {
    static const char *name() { return "longlong"; }
    static long long make(int k) { return -(long long)k; }
    static void print(long long c) { printf("%lld", c); }
};

template <typename C> struct Prob {
    int nr = 0, nc = 0;
    std::vector<int> estart, ecol;         // CSR over rows; columns of a row are distinct
    std::vector<C> ecost;
    void begin(int rows, int cols) { nr = rows; nc = cols; estart.assign(1, 0); ecol.clear(); ecost.clear(); }
    void edge(int c, C cost) { ecol.push_back(c); ecost.push_back(cost); }
    void end_row() { estart.push_back((int)ecol.size()); }
    int ne() const { return (int)ecol.size(); }
};

template <typename C> static void dump(const Prob<C> &P) {
    printf("  problem %d x %d, %d edges:", P.nr, P.nc, P.ne());
    if (P.ne() > 64) { printf(" (too large to print)\n"); return; }
    for (int r = 0; r < P.nr; ++r)
        for (int e = P.estart[r]; e < P.estart[r + 1]; ++e) { printf(" r%d-c%d:", r, P.ecol[e]); Tr<C>::print(P.ecost[e]); }
    printf("\n");
}

// the solver's arrays, each exactly as large as lap.h documents it
template <typename C> struct Solver {
    LapSmemT<C> L;
    Solver() {
        L.colmap = nullptr;                // the compaction's, not the solver's
        L.ecost = new C[LAP_EDGES]; L.u = new C[LAP_ROWS]; L.v = new C[LAP_COLS]; L.minv = new C[LAP_COLS];
        L.hrow = new int[LAP_ROWS]; L.hcol = new int[LAP_COLS]; L.estart = new int[LAP_ROWS + 1]; L.ecol = new int[LAP_EDGES];
        L.p = new int[LAP_COLS]; L.rm = new int[LAP_ROWS]; L.wayrow = new int[LAP_COLS]; L.touched = new int[LAP_COLS];
        L.usedl = new int[LAP_COLS]; L.used = new unsigned char[LAP_COLS];
    }
    ~Solver() {
        delete[] L.ecost; delete[] L.u; delete[] L.v; delete[] L.minv; delete[] L.hrow; delete[] L.hcol; delete[] L.estart;
        delete[] L.ecol; delete[] L.p; delete[] L.rm; delete[] L.wayrow; delete[] L.touched; delete[] L.usedl; delete[] L.used;
    }
    Solver(const Solver &) = delete;
    Solver &operator=(const Solver &) = delete;

    // entry state as lap_solve documents it; everything past the problem's extent holds poison, so a read of it shows
    void load(const Prob<C> &P) {
        if (P.nr > LAP_ROWS || P.nc > LAP_COLS || P.ne() > LAP_EDGES) { printf("test problem beyond the limits\n"); exit(2); }
        const C Z = LapCost<C>::zero(), INF = LapCost<C>::inf();
        for (int e = 0; e < LAP_EDGES; ++e) { L.ecol[e] = e < P.ne() ? P.ecol[e] : 0x7fffff00; L.ecost[e] = e < P.ne() ? P.ecost[e] : INF; }
        for (int h = 0; h <= LAP_ROWS; ++h) L.estart[h] = h <= P.nr ? P.estart[h] : 0x7fffff00;
        for (int h = 0; h < LAP_ROWS; ++h) { L.u[h] = h < P.nr ? Z : INF; L.rm[h] = h < P.nr ? -1 : 0x7fffff00; L.hrow[h] = h; }
        for (int j = 0; j < LAP_COLS; ++j) {
            const bool in = j < P.nc;
            L.v[j] = in ? Z : INF; L.minv[j] = in ? INF : Z; L.p[j] = in ? -1 : 0x7fffff00; L.used[j] = in ? 0 : 1;
            L.wayrow[j] = L.touched[j] = L.usedl[j] = 0x7fffff00; L.hcol[j] = j;
        }
    }

    // solves, then checks the matching (one-to-one, over given edges only, p the inverse of rm) and the post-condition
    // (minv = inf and used = 0 for every column); *obj = the sum of the matched edges' costs
    bool solve(const Prob<C> &P, C *obj) {
        load(P);
        lap_solve(L, P.nr);
        const C INF = LapCost<C>::inf();
        C sum = LapCost<C>::zero();
        std::vector<int> owner(P.nc, -1);
        for (int h = 0; h < P.nr; ++h) {
            const int j = L.rm[h];
            if (j == -1) continue;
            if (j < 0 || j >= P.nc) { printf("row %d matched to column %d of %d\n", h, j, P.nc); return false; }
            if (owner[j] >= 0) { printf("rows %d and %d share column %d\n", owner[j], h, j); return false; }
            owner[j] = h;
            int e = P.estart[h];
            while (e < P.estart[h + 1] && P.ecol[e] != j) ++e;
            if (e == P.estart[h + 1]) { printf("row %d matched to column %d without an edge\n", h, j); return false; }
            sum += P.ecost[e];
        }
        for (int j = 0; j < P.nc; ++j) {
            if (L.p[j] != owner[j]) { printf("p[%d] = %d but rm says %d\n", j, L.p[j], owner[j]); return false; }
            if (!(L.minv[j] == INF) || L.used[j] != 0) { printf("post-condition: column %d left with used %d / minv != inf\n", j, L.used[j]); return false; }
        }
        *obj = sum;
        return true;
    }

    // the optimality certificate from the solver's own duals (exact for grid costs):
    //   every edge  ecost - u - v >= 0, = 0 on matched edges;  every row  -u >= 0, = 0 on unmatched rows;  unmatched columns v = 0
    bool certificate(const Prob<C> &P) const {
        const C Z = LapCost<C>::zero();
        for (int h = 0; h < P.nr; ++h) {
            const C du = Z - L.u[h];
            if (du < Z) { printf("row %d: dummy reduced cost < 0\n", h); return false; }
            if (L.rm[h] < 0 && !(du == Z)) { printf("unmatched row %d: u != 0\n", h); return false; }
            for (int e = P.estart[h]; e < P.estart[h + 1]; ++e) {
                const int j = P.ecol[e];
                const C red = P.ecost[e] - L.u[h] - L.v[j];
                if (red < Z) { printf("edge r%d-c%d: reduced cost < 0\n", h, j); return false; }
                if (L.rm[h] == j && !(red == Z)) { printf("matched edge r%d-c%d: reduced cost != 0\n", h, j); return false; }
            }
        }
        for (int j = 0; j < P.nc; ++j)
            if (L.p[j] < 0 && !(L.v[j] == Z)) { printf("unmatched column %d: v != 0\n", j); return false; }
        return true;
    }
};

// the reference for small problems: every matching
template <typename C> static void brute(const Prob<C> &P, int r, unsigned usedmask, C cur, C *best) {
    if (r == P.nr) { if (cur < *best) *best = cur; return; }
    brute(P, r + 1, usedmask, cur, best);
    for (int e = P.estart[r]; e < P.estart[r + 1]; ++e) {
        const int j = P.ecol[e];
        if (usedmask >> j & 1) continue;
        brute(P, r + 1, usedmask | 1u << j, cur + P.ecost[e], best);
    }
}

template <typename C> static bool small_case(Solver<C> &S, const Prob<C> &P, const char *family) {
    C got, best = LapCost<C>::zero();
    const bool ok = S.solve(P, &got) && S.certificate(P);
    brute(P, 0, 0u, LapCost<C>::zero(), &best);
    if (!ok || !(got == best)) {
        printf("%s %s: ", family, Tr<C>::name());
        if (ok) { printf("objective "); Tr<C>::print(got); printf(", every-matching optimum "); Tr<C>::print(best); printf("\n"); }
        dump(P);
        return false;
    }
    return true;
}

// pattern bit r * nc + c = edge (r, c); gains drawn by gain(edge index)
template <typename C, typename G> static void from_pattern(Prob<C> &P, int nr, int nc, unsigned long long pat, G gain) {
    P.begin(nr, nc);
    int idx = 0;
    for (int r = 0; r < nr; ++r) {
        for (int c = 0; c < nc; ++c)
            if (pat >> (r * nc + c) & 1) P.edge(c, Tr<C>::make(gain(idx++)));
        P.end_row();
    }
}

template <typename C> static int check_exhaustive() {
    Solver<C> S;
    Prob<C> P;
    std::mt19937_64 rng(20240611);
    long n = 0;
    for (int nr = 1; nr <= 4; ++nr)
        for (int nc = 1; nc <= 4; ++nc)
            for (unsigned long long pat = 0; pat < (1ull << (nr * nc)); ++pat) {
                const int ne = __builtin_popcountll(pat);
                if (nr * nc <= 9) {                            // every cost assignment from {1, 2}
                    for (unsigned cm = 0; cm < (1u << ne); ++cm) {
                        from_pattern(P, nr, nc, pat, [&](int i) { return 1 + (int)(cm >> i & 1); });
                        if (!small_case(S, P, "exhaustive")) return 1;
                        ++n;
                    }
                } else {                                       // all equal, then draws from {1, 2, 3}
                    for (int t = 0; t < 4; ++t) {
                        from_pattern(P, nr, nc, pat, [&](int) { return t == 0 ? 2 : 1 + (int)(rng() % 3); });
                        if (!small_case(S, P, "exhaustive")) return 1;
                        ++n;
                    }
                }
            }
    printf("ok exhaustive %s %ld graphs up to 4x4\n", Tr<C>::name(), n);
    return 0;
}

template <typename C> static int check_random_small() {
    Solver<C> S;
    Prob<C> P;
    std::mt19937_64 rng(77);
    const int N = 4000;
    for (int t = 0; t < N; ++t) {
        const int nr = 1 + (int)(rng() % 7), nc = 1 + (int)(rng() % 7), K = 1 + (int)(rng() % 5);
        const unsigned dens = 15 + (unsigned)(rng() % 70);
        unsigned long long pat = 0;
        for (int b = 0; b < nr * nc; ++b) if (rng() % 100 < dens) pat |= 1ull << b;
        from_pattern(P, nr, nc, pat, [&](int) { return 1 + (int)(rng() % K); });
        if (!small_case(S, P, "random-small")) return 1;
    }
    printf("ok random-small %s %d graphs up to 7x7\n", Tr<C>::name(), N);
    return 0;
}

// large structured graphs: validity, post-condition, certificate; `expect` (or nullptr) = the unique optimum's rm
template <typename C> static bool big_case(Solver<C> &S, const Prob<C> &P, const char *family, const std::vector<int> *expect = nullptr) {
    C got;
    if (!S.solve(P, &got) || !S.certificate(P)) { printf("%s %s\n", family, Tr<C>::name()); dump(P); return false; }
    if (expect)
        for (int h = 0; h < P.nr; ++h)
            if (S.L.rm[h] != (*expect)[h]) { printf("%s %s: row %d -> %d, expected %d\n", family, Tr<C>::name(), h, S.L.rm[h], (*expect)[h]); return false; }
    return true;
}

// r_i - c_i (gain 512) and r_i - c_{i+1} (gain 513); the last row has c_{n-1} only (gain 1000): rows 0..n-2 take c_{i+1}, and
// solving the last row shifts every one of them back (one augmenting path through all n rows)
template <typename C> static int check_chain() {
    Solver<C> S;
    Prob<C> P;
    for (int n : {2, 3, 64, 255, 256}) {
        P.begin(n, n);
        for (int i = 0; i < n; ++i) {
            P.edge(i, Tr<C>::make(i == n - 1 ? 1000 : 512));
            if (i + 1 < n) P.edge(i + 1, Tr<C>::make(513));
            P.end_row();
        }
        std::vector<int> expect(n);
        for (int i = 0; i < n; ++i) expect[i] = i;
        if (!big_case(S, P, "chain", &expect)) return 1;
    }
    printf("ok chain %s re-routed through 256 rows\n", Tr<C>::name());
    return 0;
}

// n rows, n - 1 columns: r_0 - c_0 (gain 300); r_i - c_{i-1} (gain 501) and r_i - c_i (gain 500); the last row has c_{n-2} only
// (gain 600).  Rows 0..n-2 take c_i; the last row's best move shifts every row down one column and evicts row 0 to its
// dummy (gain 600 + (n - 2) - 300; stopping at row k > 0 gains 354 - k at most at n = 256): the to_dummy branch, full length
template <typename C> static int check_chain_evict() {
    Solver<C> S;
    Prob<C> P;
    for (int n : {2, 3, 64, 255, 256}) {
        P.begin(n, n - 1);
        for (int i = 0; i < n; ++i) {
            if (i > 0) P.edge(i - 1, Tr<C>::make(i == n - 1 ? 600 : 501));
            if (i < n - 1) P.edge(i, Tr<C>::make(i == 0 ? 300 : 500));
            P.end_row();
        }
        std::vector<int> expect(n);
        for (int i = 0; i < n; ++i) expect[i] = i - 1;
        if (!big_case(S, P, "chain-evict", &expect)) return 1;
    }
    printf("ok chain-evict %s first row evicted through 256 rows\n", Tr<C>::name());
    return 0;
}

template <typename C> static int check_star() {
    Solver<C> S;
    Prob<C> P;
    std::mt19937_64 rng(5);
    for (int variant = 0; variant < 3; ++variant) {            // gains ascending (every row evicts the last), descending, shuffled
        std::vector<int> g(LAP_ROWS);
        for (int i = 0; i < LAP_ROWS; ++i) g[i] = variant == 1 ? 700 - i : 100 + i;
        if (variant == 2) std::shuffle(g.begin(), g.end(), rng);
        P.begin(LAP_ROWS, 1);
        for (int i = 0; i < LAP_ROWS; ++i) { P.edge(0, Tr<C>::make(g[i])); P.end_row(); }
        std::vector<int> expect(LAP_ROWS, -1);
        expect[std::max_element(g.begin(), g.end()) - g.begin()] = 0;
        if (!big_case(S, P, "star", &expect)) return 1;
    }
    printf("ok star %s 256 rows on one column\n", Tr<C>::name());
    return 0;
}

template <typename C> static int check_star_t() {
    Solver<C> S;
    Prob<C> P;
    std::mt19937_64 rng(6);
    for (int variant = 0; variant < 3; ++variant) {
        std::vector<int> g(LAP_COLS);
        for (int i = 0; i < LAP_COLS; ++i) g[i] = variant == 1 ? 700 - i : 100 + i;
        if (variant == 2) std::shuffle(g.begin(), g.end(), rng);
        P.begin(1, LAP_COLS);
        for (int j = 0; j < LAP_COLS; ++j) P.edge(j, Tr<C>::make(g[j]));
        P.end_row();
        std::vector<int> expect(1, (int)(std::max_element(g.begin(), g.end()) - g.begin()));
        if (!big_case(S, P, "star-transposed", &expect)) return 1;
    }
    printf("ok star-transposed %s one row on 256 columns\n", Tr<C>::name());
    return 0;
}

template <typename C, typename G> static void complete(Prob<C> &P, int nr, int nc, G gain) {
    P.begin(nr, nc);
    for (int r = 0; r < nr; ++r) { for (int c = 0; c < nc; ++c) P.edge(c, Tr<C>::make(gain())); P.end_row(); }
}

// every row has column (row * 97 % 256) -- so all 256 columns occur -- and 7 more distinct ones: 256 / 256 / 2048 exactly
template <typename C, typename G> static void sparse_limit(Prob<C> &P, std::mt19937_64 &rng, G gain) {
    P.begin(LAP_ROWS, LAP_COLS);
    for (int r = 0; r < LAP_ROWS; ++r) {
        std::vector<int> cols(1, r * 97 % LAP_COLS);
        while ((int)cols.size() < LAP_EDGES / LAP_ROWS) {
            const int c = (int)(rng() % LAP_COLS);
            if (std::find(cols.begin(), cols.end(), c) == cols.end()) cols.push_back(c);
        }
        std::sort(cols.begin(), cols.end());
        for (int c : cols) P.edge(c, Tr<C>::make(gain()));
        P.end_row();
    }
}

template <typename C> static int check_complete45() {
    Solver<C> S;
    Prob<C> P;
    std::mt19937_64 rng(45);
    for (int t = 0; t < 6; ++t) {
        const int K = t < 3 ? 1023 : 4;                        // generic, then heavy ties
        complete(P, 45, 45, [&] { return 1 + (int)(rng() % K); });
        if (!big_case(S, P, "complete45")) return 1;
    }
    printf("ok complete45 %s 45 x 45 = 2025 edges\n", Tr<C>::name());
    return 0;
}

template <typename C> static int check_complete256x8() {
    Solver<C> S;
    Prob<C> P;
    std::mt19937_64 rng(2568);
    for (int t = 0; t < 6; ++t) {
        const int K = t < 3 ? 1023 : 4;
        complete(P, LAP_ROWS, 8, [&] { return 1 + (int)(rng() % K); });
        if (P.ne() != LAP_EDGES || !big_case(S, P, "complete256x8")) return 1;
    }
    complete(P, 8, LAP_COLS, [&] { return 1 + (int)(rng() % 1023); });       // and its transpose
    if (P.ne() != LAP_EDGES || !big_case(S, P, "complete8x256")) return 1;
    printf("ok complete256x8 %s 2048 edges, the limit\n", Tr<C>::name());
    return 0;
}

template <typename C> static int check_sparse_limit() {
    Solver<C> S;
    Prob<C> P;
    std::mt19937_64 rng(256256);
    for (int t = 0; t < 8; ++t) {
        const int K = t < 4 ? 1023 : 6;
        sparse_limit(P, rng, [&] { return 1 + (int)(rng() % K); });
        std::vector<char> seen(LAP_COLS, 0);
        for (int c : P.ecol) seen[c] = 1;
        if (P.nr != LAP_ROWS || P.ne() != LAP_EDGES || std::count(seen.begin(), seen.end(), 1) != LAP_COLS) { printf("sparse-limit: not at the limits\n"); return 1; }
        if (!big_case(S, P, "sparse-limit")) return 1;
    }
    printf("ok sparse-limit %s 256 rows / 256 columns / 2048 edges\n", Tr<C>::name());
    return 0;
}

template <typename C> static int check_equal() {
    Solver<C> S;
    Prob<C> P;
    std::mt19937_64 rng(3);
    complete(P, 45, 45, [] { return 500; });
    if (!big_case(S, P, "all-equal")) return 1;
    complete(P, LAP_ROWS, 8, [] { return 500; });
    if (!big_case(S, P, "all-equal")) return 1;
    sparse_limit(P, rng, [] { return 500; });
    if (!big_case(S, P, "all-equal")) return 1;
    P.begin(LAP_ROWS, LAP_COLS);                               // the chain with nothing to choose between
    for (int i = 0; i < LAP_ROWS; ++i) { P.edge(i, Tr<C>::make(500)); if (i + 1 < LAP_COLS) P.edge(i + 1, Tr<C>::make(500)); P.end_row(); }
    if (!big_case(S, P, "all-equal")) return 1;
    printf("ok all-equal %s complete, limit-sized and chain graphs\n", Tr<C>::name());
    return 0;
}

template <typename C> static int check_type() {
    return check_exhaustive<C>() || check_random_small<C>() || check_chain<C>() || check_chain_evict<C>() || check_star<C>() ||
           check_star_t<C>() || check_complete45<C>() || check_complete256x8<C>() || check_sparse_limit<C>() || check_equal<C>();
}

// "<count>", then per problem "<nr> <nc> <ne>", nr + 1 row starts, ne columns, ne costs (hexadecimal floats: exact)
static int check_file(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) { printf("cannot open %s\n", path); return 1; }
    Solver<double> S;
    Prob<double> P;
    int count = 0;
    if (fscanf(f, "%d", &count) != 1) { printf("bad problem file\n"); fclose(f); return 1; }
    for (int i = 0; i < count; ++i) {
        int nr, nc, ne;
        if (fscanf(f, "%d %d %d", &nr, &nc, &ne) != 3 || nr < 0 || nc < 0 || ne < 0) { printf("bad problem %d\n", i); fclose(f); return 1; }
        P.nr = nr; P.nc = nc;
        P.estart.assign(nr + 1, 0); P.ecol.assign(ne, 0); P.ecost.assign(ne, 0.0);
        bool ok = true;
        for (int &x : P.estart) ok = ok && fscanf(f, "%d", &x) == 1;
        for (int &x : P.ecol) ok = ok && fscanf(f, "%d", &x) == 1;
        for (double &x : P.ecost) ok = ok && fscanf(f, "%la", &x) == 1;
        if (!ok || P.estart[nr] != ne) { printf("bad problem %d\n", i); fclose(f); return 1; }
        double obj;
        if (!S.solve(P, &obj)) { printf("file problem %d\n", i); fclose(f); return 1; }
        printf("obj %d %.17g\n", i, obj);
    }
    fclose(f);
    printf("ok file double %d generic problems solved\n", count);
    return 0;
}

int main(int argc, char **argv) {
    if (check_type<double>() || check_type<LexCost>() || check_type<long long>()) return 1;
    if (argc > 1 && check_file(argv[1])) return 1;
    return 0;
}
