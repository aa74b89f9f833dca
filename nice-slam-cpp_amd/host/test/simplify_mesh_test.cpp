// simplify_mesh_test.cpp -- driver of Mesher::simplify_mesh for tests/test_gpu_simplify.py.
//   simplify_mesh_test IN.ply OUT.ply CELL [keep_duplicates]
//        OUT.ply: IN.ply clustered on a uniform grid of edge CELL (the PLY -> PLY overload);  one JSON line on stdout
#include <cstdio>
#include <cstdlib>
#include <string>

#include "Mesher.h"

int main(int argc, char** argv)
{
    if (argc != 4 && argc != 5) { std::fprintf(stderr, "usage: simplify_mesh_test IN.ply OUT.ply CELL [keep_duplicates]\n"); return 2; }
    try {
        const float cell = (float)std::atof(argv[3]);
        const bool keep = argc == 5 && std::string(argv[4]) != "0";
        const SimplifiedMesh R = Mesher::simplify_mesh(argv[1], argv[2], cell, keep);
        long long mapped = 0;
        for (int32_t m : R.vertex_map) mapped += m >= 0;
        std::printf("{\"cell\": %.9g, \"keep_duplicates\": %d, \"in_vertices\": %zu, \"vertices\": %zu, \"triangles\": %zu, \"mapped\": %lld, "
                    "\"finite\": %lld, \"left_out\": %lld, \"invalid\": %lld, \"collapsed\": %lld, \"duplicates\": %lld, \"occupied\": %lld, "
                    "\"cells\": %lld, \"dims\": [%lld, %lld, %lld]}\n", (double)cell, keep ? 1 : 0, R.vertex_map.size(), R.xyz.size() / 3,
                    R.triangles.size() / 3, mapped, R.info[0], R.info[1], R.info[2], R.info[3], R.info[4], R.info[5], R.info[6],
                    R.info[7] & 0x1fffff, (R.info[7] >> 21) & 0x1fffff, (R.info[7] >> 42) & 0x1fffff);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "simplify_mesh_test failed: %s\n", e.what());
        return 1;
    }
}
