// crosscam_rule_check.cpp -- csrc/crosscam_rule.h as a stand-alone host program (tests/test_crosscam_cpu.py builds it plain and under
// the address / undefined-behaviour sanitizers and compares its output, line by line, with tests/crosscam_ref.py on the same inputs).
// stdin, one request per line:
//   sim dot nq ng                      -> the similarity per mille
//   transit c last tmin tmax           -> 0 / 1
//   feat birth dim s16[dim] f[dim]     -> s16[dim] s8[dim] after one step (birth 1: s16 is ignored)
//   isqrt n                            -> floor(sqrt(n))
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "crosscam_rule.h"

int main() {
    std::string op;
    while (std::cin >> op) {
        if (op == "sim") {
            long long dot, nq, ng;
            std::cin >> dot >> nq >> ng;
            std::printf("%d\n", rtmodt::cc_sim((int32_t)dot, nq, ng));
        } else if (op == "transit") {
            long long c, last; int lo, hi;
            std::cin >> c >> last >> lo >> hi;
            std::printf("%d\n", rtmodt::cc_transit_ok(c, last, lo, hi) ? 1 : 0);
        } else if (op == "isqrt") {
            long long n;
            std::cin >> n;
            std::printf("%lld\n", rtmodt::cc_isqrt(n));
        } else if (op == "feat") {
            int birth, dim;
            std::cin >> birth >> dim;
            if (dim < 1 || dim > rtmodt::CC_MAX_DIM) return 2;
            std::vector<int16_t> s16(dim);
            std::vector<int8_t> s8(dim), f(dim);
            for (int k = 0; k < dim; ++k) { int v; std::cin >> v; s16[k] = (int16_t)v; }
            for (int k = 0; k < dim; ++k) { int v; std::cin >> v; f[k] = (int8_t)v; }
            rtmodt::cc_feat_step(birth != 0, s16.data(), s8.data(), f.data(), dim);
            for (int k = 0; k < dim; ++k) std::printf("%d ", (int)s16[k]);
            for (int k = 0; k < dim; ++k) std::printf("%d%c", (int)s8[k], k + 1 == dim ? '\n' : ' ');
        } else {
            return 3;
        }
    }
    return 0;
}
