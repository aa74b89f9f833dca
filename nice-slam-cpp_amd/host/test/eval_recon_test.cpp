// eval_recon_test REC.ply GT.ply [n] [threshold] [seed] [align] [surface] -- Mesher::eval_recon on two PLY files, one JSON line
// (tests/test_gpu_recon.py, tests/test_gpu_icp.py, tests/test_gpu_surface.py); align 1: the reconstruction is registered to the ground truth
// first and the alignment is printed too; surface (given at all: 1 measures against the other mesh, 0 against its samples): the surface
// fields are printed too
#include <cstdio>
#include <cstdlib>
#include <exception>

#include "Mesher.h"

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s REC.ply GT.ply [n] [threshold] [seed] [align] [surface]\n", argv[0]); return 2; }
    const int n = argc > 3 ? std::atoi(argv[3]) : 200000;
    const float threshold = argc > 4 ? (float)std::atof(argv[4]) : 0.05f;
    const unsigned long long seed = argc > 5 ? std::strtoull(argv[5], nullptr, 10) : 0ull;
    const bool align = argc > 6 && std::atoi(argv[6]) != 0;
    const bool has_surface = argc > 7, surface = has_surface && std::atoi(argv[7]) != 0;
    try {
        const ReconMetrics m = Mesher::eval_recon(argv[1], argv[2], n, threshold, seed, align, surface);
        std::printf("{\"accuracy_cm\": %.17g, \"completion_cm\": %.17g, \"completion_ratio_pct\": %.17g, \"accuracy_max_cm\": %.17g, "
                    "\"completion_max_cm\": %.17g, \"rec_area\": %.17g, \"gt_area\": %.17g, \"rec_degenerate\": %d, \"gt_degenerate\": %d, "
                    "\"rec_skipped\": %d, \"gt_skipped\": %d, \"n\": %d, \"threshold\": %.9g",
                    m.accuracy_cm, m.completion_cm, m.completion_ratio_pct, m.accuracy_max_cm, m.completion_max_cm, m.rec_area, m.gt_area,
                    m.rec_degenerate, m.gt_degenerate, m.rec_skipped, m.gt_skipped, n, (double)threshold);
        if (align) {
            std::printf(", \"icp_fitness\": %.17g, \"icp_rmse\": %.17g, \"icp_iterations\": %d, \"transform\": [", m.icp_fitness, m.icp_rmse, m.icp_iterations);
            for (int k = 0; k < 16; ++k) std::printf("%s%.17g", k ? ", " : "", m.transform[k]);
            std::printf("]");
        }
        if (has_surface)
            std::printf(", \"surface\": %s, \"precision_pct\": %.17g, \"recall_pct\": %.17g, \"fscore_pct\": %.17g, \"normal_accuracy\": %.17g, "
                        "\"normal_completion\": %.17g, \"normal_consistency\": %.17g, \"normal_skipped\": %d", m.surface ? "true" : "false",
                        m.precision_pct, m.recall_pct, m.fscore_pct, m.normal_accuracy, m.normal_completion, m.normal_consistency, m.normal_skipped);
        std::printf("}\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "eval_recon_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
