// Prints what csrc/gemv_instance.hpp selects for every shape named on the command line, one line per (shape, pairing, LayerNorm form, scale form):
//     rows cols paired ln sc wscale | ok k_split ks_log2 blocks blocks_per_wave ring nv ln_inst merge tiles_per_wg grid lds raise
// tests/test_gemv_mfma_ref.py restates the selection as launch_gemv_mfma made it before it moved into that header and compares line by line.
// argv: rows... "x" blocks_lo blocks_hi.  Plain host C++: the header needs no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gemv_instance.hpp"

int main(int argc, char **argv) {
    std::vector<size_t> rows;
    int i = 1;
    for (; i < argc && std::strcmp(argv[i], "x") != 0; ++i) rows.push_back((size_t)std::atoll(argv[i]));
    if (i + 2 >= argc) return 2;
    const int lo = std::atoi(argv[i + 1]), hi = std::atoi(argv[i + 2]);
    for (size_t r : rows)
        for (int nblk = lo; nblk <= hi; ++nblk)
            for (int paired = 0; paired < 2; ++paired)
                for (int ln = 0; ln < 3; ++ln)
                    for (int sc = 0; sc < 4; ++sc) {  // 3 = no 32-block scales, 256-block scales
                        bitnet_hip::GemvShape s;
                        s.rows = r;
                        s.cols = (size_t)nblk * 256;
                        s.sc = sc == 3 ? 0 : sc;
                        s.wscale = sc == 3;
                        bitnet_hip::GemvMfmaInstance q;
                        const bool ok = bitnet_hip::gemv_mfma_instance(s, paired != 0, ln != 0, ln == 2, false, 1, q);
                        std::printf("%zu %zu %d %d %d %d |", s.rows, s.cols, paired, ln, s.sc, (int)s.wscale);
                        if (!ok)
                            std::printf(" 0\n");
                        else
                            std::printf(" 1 %d %d %d %d %d %d %d %d %d %u %zu %d\n", q.g.ksplit, q.g.ks_log2, q.g.nblk, q.g.ring, q.ring_inst, q.nv_inst, q.ln,
                                        q.merge, q.g.tiles_per_wg, q.g.grid, q.lds, (int)q.raise_lds);
                    }
    // the merging form: 48 rows, every block count, every scale form
    for (int nblk = lo; nblk <= hi; ++nblk)
        for (int sc = 0; sc < 3; ++sc) {
            bitnet_hip::GemvShape s{48, (size_t)nblk * 256, sc, false};
            bitnet_hip::GemvMfmaInstance q;
            const bool ok = bitnet_hip::gemv_mfma_instance(s, false, false, false, true, 1, q);
            std::printf("merge %d %d | %d", nblk, sc, (int)ok);
            if (ok) std::printf(" %d %d %d %d %d %zu", q.g.ksplit, q.g.ring, q.ring_inst, q.nv_inst, q.merge, q.lds);
            std::printf("\n");
        }
    return 0;
}
