// host_amg_test.cpp -- driver of tests/test_host_amg.py: reads one CSR matrix (with an exclusion mask and a payload of `width` doubles per entry), runs
// host_coarsen (csrc/host_amg.cpp) without and with absorption, and writes everything it built.  Plain C++: no GPU.
//   usage: host_amg_test IN OUT0 OUT1
//   IN    int32 n, nnz, width, has_excl; int32 rp[n + 1], ci[nnz]; double a[nnz]; double pay[width nnz]; uint8 excl[n] if has_excl
//   OUTk  (absorb = k) int32 n1, n2, nnzT, nnzN; int32 agg1[n], agg2[n1], agg[n], mptr[n2 + 1], midx[mptr[n2]];
//         int32 T.rp[n1 + 1], T.ci[nnzT]; double T.a[nnzT], payT[width nnzT]; int32 N.rp[n2 + 1], N.ci[nnzN]; double N.a[nnzN], payN[width nnzN]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../fdapde-core_amd/csrc/amg_rows.h"

using namespace fdapde_engine;

template <typename T> static bool rd(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T> static bool wr(std::FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    std::vector<int32_t> hdr;
    if (!f || !rd(f, hdr, 4)) return 3;
    const size_t n = (size_t)hdr[0], nnz = (size_t)hdr[1];
    const int width = hdr[2];
    HostCsr A;
    std::vector<double> pay;
    std::vector<uint8_t> excl;
    A.n = hdr[0];
    if (!rd(f, A.rp, n + 1) || !rd(f, A.ci, nnz) || !rd(f, A.a, nnz) || !rd(f, pay, (size_t)width * nnz) || !rd(f, excl, hdr[3] ? n : 0)) return 3;
    std::fclose(f);
    for (int absorb = 0; absorb < 2; ++absorb) {
        HostCoarse h;
        host_coarsen(A, hdr[3] ? excl.data() : nullptr, absorb, width ? pay.data() : nullptr, width, h);
        std::FILE* o = std::fopen(argv[2 + absorb], "wb");
        const std::vector<int32_t> head{h.n1, h.n2, (int32_t)h.T.ci.size(), (int32_t)h.N.ci.size()};
        if (!o || !wr(o, head) || !wr(o, h.agg1) || !wr(o, h.agg2) || !wr(o, h.agg) || !wr(o, h.mptr) || !wr(o, h.midx) || !wr(o, h.T.rp) || !wr(o, h.T.ci) ||
            !wr(o, h.T.a) || !wr(o, h.payT) || !wr(o, h.N.rp) || !wr(o, h.N.ci) || !wr(o, h.N.a) || !wr(o, h.payN))
            return 4;
        std::fclose(o);
        std::printf("ok absorb %d: %zu rows -> %d -> %d\n", absorb, n, h.n1, h.n2);
    }
    return 0;
}
