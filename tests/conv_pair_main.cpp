// Stand-alone driver of csrc/gemm_route.cpp for tests/test_cpu_conv_pair_check.py: links that unit alone (nothing from HIP, so nothing can
// launch).  First line: sizeof(toist_conv_pair) and the offset of every field, in declaration order.  Then it reads consecutive raw
// toist_conv_pair structs from the file named on the command line and prints one line per descriptor:
//   code applies family-of-the-second-product | message
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../toist_amd/csrc/gemm_route.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
#define OFF(f) offsetof(toist_conv_pair, f)
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(toist_conv_pair), OFF(M), OFF(C), OFF(dgrad),
                OFF(lda), OFF(a), OFF(w_first), OFF(w_second), OFF(shift_mid), OFF(shift_out), OFF(res), OFF(aux_mid), OFF(aux_out), OFF(mid), OFF(out),
                OFF(ldr), OFF(ldaux_mid), OFF(ldaux_out), OFF(ldmid), OFF(ldout), OFF(reserved));
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<toist_conv_pair> descs;
    toist_conv_pair d;
    while (std::fread(&d, sizeof(d), 1, f) == 1) descs.push_back(d);
    std::fclose(f);
    for (const toist_conv_pair& desc : descs) {
        const toist::gemm_verdict v = toist::pair_check(desc);
        const int family = v.code == TOIST_OK ? toist::gemm_route(toist::pair_second_gemm(desc)).family : -1;
        std::printf("%d %d %d | %s\n", v.code, toist::pair_applies(desc) ? 1 : 0, family, v.msg);
    }
    return 0;
}
