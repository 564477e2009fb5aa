// Host-side check of the JPEG decoder's stream side (csrc/jpeg_dec_core.h: jd_parse, jd_decode_interval), compiled by
// tests/test_jpeg_dec_cpu.py (once plain, once with the address and undefined-behaviour sanitizers).  Every buffer is a heap block
// of exactly its documented size -- the file's bytes, the frame's blocks x 64 int16 -- so a read or write one past an end is a
// heap overrun the sanitizer reports.
//
//   jpeg_dec_check list.txt       list.txt: one "<path> <expected status, or -1>" per line
//
// hash = sum over i of (uint16(v_i) + 1) * ((i + 1) * 0x9E3779B97F4A7C15) mod 2^64 over the int16 coefficients, component after component.
// One line "<index> <status> <hash of the coefficients; 0 unless OK>" per file.  Exit code 1
// if a status differs from the expected one, 2 on a usage / IO error, else 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "jpeg_dec_core.h"
using namespace rtmodt;

static int decode_file(const uint8_t *d, size_t n, unsigned long long &hash) {
    hash = 0;
    JdHeader *hd = (JdHeader *)calloc(1, sizeof(JdHeader));
    const char *msg = nullptr;
    int status = jd_parse(d, n, *hd, &msg);
    if (status != JD_OK) {
        free(hd);
        return status;
    }
    JdLayout lay;
    const size_t blocks = jd_layout(*hd, lay);
    int16_t *coef = (int16_t *)calloc(blocks * 64, sizeof(int16_t));
    uint8_t zz[64];
    jd_zigzag_fill(zz);
    // the restart markers of the scan, in stream order
    std::vector<uint32_t> marks;
    for (uint32_t p = hd->scan_off; p + 1 < hd->scan_end; ++p)
        if (d[p] == 0xFF && d[p + 1] >= 0xD0 && d[p + 1] <= 0xD7) marks.push_back(p);
    if ((long long)marks.size() != (long long)hd->intervals - 1) {
        status = JD_CORRUPT;
    } else {
        const long long mcus = (long long)hd->mcus_x * hd->mcus_y, per = hd->ri ? hd->ri : mcus;
        for (int j = 0; j < hd->intervals; ++j) {
            const uint32_t start = j == 0 ? hd->scan_off : marks[j - 1] + 2, end = j == hd->intervals - 1 ? hd->scan_end : marks[j];
            int st;
            if (j && (d[marks[j - 1] + 1] & 7) != ((j - 1) & 7)) {
                st = JD_CORRUPT;
            } else {
                const long long first = (long long)j * per, count = first + per <= mcus ? per : mcus - first;
                st = jd_decode_interval(d + start, d + end, *hd, hd->huff, zz, lay, first, count, coef);
            }
            if (st > status) status = st;
        }
    }
    if (status == JD_OK) {
        unsigned long long h = 0;
        for (size_t i = 0; i < blocks * 64; ++i) h += ((unsigned long long)(uint16_t)coef[i] + 1ull) * ((i + 1ull) * 0x9E3779B97F4A7C15ull);
        hash = h;
    }
    free(coef);
    free(hd);
    return status;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: jpeg_dec_check list.txt\n");
        return 2;
    }
    FILE *lf = fopen(argv[1], "r");
    if (!lf) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    char path[4096];
    int expected, index = 0, wrong = 0;
    while (fscanf(lf, "%4095s %d", path, &expected) == 2) {
        FILE *f = fopen(path, "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", path);
            return 2;
        }
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t *d = (uint8_t *)malloc(n > 0 ? (size_t)n : 1);        // exactly the file: nothing behind it may be read
        if (n > 0 && fread(d, 1, (size_t)n, f) != (size_t)n) {
            fprintf(stderr, "cannot read %s\n", path);
            return 2;
        }
        fclose(f);
        unsigned long long hash;
        const int status = decode_file(d, (size_t)n, hash);
        free(d);
        printf("%d %d %016llx\n", index, status, hash);
        if (expected >= 0 && status != expected) {
            fprintf(stderr, "%s: status %d, expected %d\n", path, status, expected);
            ++wrong;
        }
        ++index;
    }
    fclose(lf);
    return wrong ? 1 : 0;
}
