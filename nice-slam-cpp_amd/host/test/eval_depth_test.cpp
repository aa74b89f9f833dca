// eval_depth_test REC.ply GT.ply N_VIEWS H W FOCAL SEED [ALIGN] -- Mesher::eval_recon_depth on two PLY files, one JSON line
// (tests/test_gpu_raster.py, tests/test_gpu_icp.py); ALIGN 1: the reconstruction is registered to the ground truth first
#include <cstdio>
#include <cstdlib>
#include <exception>

#include "Mesher.h"

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s REC.ply GT.ply [N_VIEWS] [H] [W] [FOCAL] [SEED] [ALIGN]\n", argv[0]); return 2; }
    const int n_views = argc > 3 ? std::atoi(argv[3]) : 1000;
    const int H = argc > 4 ? std::atoi(argv[4]) : 500, W = argc > 5 ? std::atoi(argv[5]) : 500;
    const float focal = argc > 6 ? (float)std::atof(argv[6]) : 300.f;
    const unsigned long long seed = argc > 7 ? std::strtoull(argv[7], nullptr, 10) : 0ull;
    const bool align = argc > 8 && std::atoi(argv[8]) != 0;
    try {
        const ReconDepth m = Mesher::eval_recon_depth(argv[1], argv[2], n_views, H, W, focal, seed, 0.7, 0.0, align);
        std::printf("{\"depth_l1_cm\": %.17g, \"restricted_l1_cm\": %.17g, \"n_views\": %d, \"n_used\": %d, \"rec_skipped\": %d, "
                    "\"gt_skipped\": %d, \"H\": %d, \"W\": %d, \"focal\": %.9g, \"view0_l1\": %.17g, \"w2c0\": [",
                    m.depth_l1_cm, m.restricted_l1_cm, m.n_views, m.n_used, m.rec_skipped, m.gt_skipped, H, W, (double)focal, m.view_l1[0]);
        for (int k = 0; k < 16; ++k) std::printf("%s%.9g", k ? ", " : "", (double)m.w2c[k]);
        std::printf("]");
        if (align) {
            std::printf(", \"icp_fitness\": %.17g, \"icp_rmse\": %.17g, \"icp_iterations\": %d, \"transform\": [", m.icp_fitness, m.icp_rmse, m.icp_iterations);
            for (int k = 0; k < 16; ++k) std::printf("%s%.17g", k ? ", " : "", m.transform[k]);
            std::printf("]");
        }
        std::printf("}\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "eval_depth_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
