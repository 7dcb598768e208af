// Stand-alone driver of csrc/gemm_route.cpp for tests/test_cpu_gemm_route.py: links that unit alone (nothing from HIP, so nothing can
// launch), reads consecutive raw toist_gemm structs from the file named on the command line and prints one line per descriptor:
//   code family tile ring split post | route-with-workspace split | toist_gemm_pick_tile toist_gemm_effective_split | message
#include <cstdio>
#include <vector>

#include "../toist_amd/csrc/gemm_route.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<toist_gemm> descs;
    toist_gemm d;
    while (std::fread(&d, sizeof(d), 1, f) == 1) descs.push_back(d);
    std::fclose(f);
    for (const toist_gemm& desc : descs) {
        const toist::gemm_verdict v = toist::gemm_check(desc);
        const toist::gemm_plan r = toist::gemm_route(desc);
        toist_gemm w = desc;
        if (w.workspace == nullptr) w.workspace = (float*)16;      // toist_gemm_effective_split's assumption
        const toist::gemm_verdict& said = v.code != TOIST_OK ? v : static_cast<const toist::gemm_verdict&>(r);
        std::printf("%d %d %d %d %d %d | %d | %d %d | %s\n", said.code, r.family, r.tile, r.ring, r.split, r.post, toist::gemm_route(w).split,
                    toist_gemm_pick_tile(&desc), toist_gemm_effective_split(&desc), said.msg);
    }
    return 0;
}
