// delaunay_predicates_main.cpp -- runs the predicates of csrc/csplat_delaunay_predicates.h on the host: test_delaunay_cpu.py compiles this
// with the host compiler, feeds it tests/delaunay_ref.py's adversarial inputs and compares every sign with integer arithmetic.
//   usage: delaunay_predicates_main <records in> <signs out>
// in:  int32 count, then per record 13 32-bit words: kind (0 orientation, 1 distance, 2 in-circle), four point indices, four points as
//      float32 (x, y).  out: per record two int32: the sign, and whether the exact stage took the decision.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "csplat_delaunay_predicates.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 3;
    int32_t count = 0;
    if (fread(&count, 4, 1, in) != 1 || count < 0) return 4;
    std::vector<int32_t> words((size_t)count * 13), out((size_t)count * 2);
    if (fread(words.data(), 4, words.size(), in) != words.size()) return 5;
    fclose(in);
    for (int32_t r = 0; r < count; r++) {
        const int32_t *w = &words[(size_t)r * 13];
        float xy[8];
        memcpy(xy, w + 5, sizeof(xy));
        dp_pt p[4];
        for (int q = 0; q < 4; q++) p[q] = dp_pt{(double)xy[2 * q], (double)xy[2 * q + 1]};
        unsigned exact = 0;
        int s;
        if (w[0] == 0) s = dp_orient(p[0], p[1], p[2], exact);
        else if (w[0] == 1) s = dp_nearer(p[0], p[1], p[2], exact);
        else s = dp_incircle(p[0], p[1], p[2], p[3], w[1], w[2], w[3], w[4], exact);
        out[(size_t)r * 2] = s, out[(size_t)r * 2 + 1] = (int32_t)exact;
    }
    FILE *of = fopen(argv[2], "wb");
    if (!of) return 6;
    if (fwrite(out.data(), 4, out.size(), of) != out.size()) return 7;
    fclose(of);
    return 0;
}
