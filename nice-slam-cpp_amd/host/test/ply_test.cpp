// ply_test FILE.ply ... -- Mesher::read_ply_mesh on each file (no GPU).  Per file: "file PATH", then "nv nt", the vertices and the triangles
// as text, or "error MESSAGE" where the reader threw (tests/test_ply_reader.py)
#include <cstdio>
#include <exception>

#include "Mesher.h"

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s FILE.ply ...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        std::vector<float> xyz;
        std::vector<int32_t> tris;
        std::printf("file %s\n", argv[a]);
        try {
            Mesher::read_ply_mesh(argv[a], xyz, tris);
        } catch (const std::exception& e) {
            std::printf("error %s\n", e.what());
            continue;
        }
        std::printf("%zu %zu\n", xyz.size() / 3, tris.size() / 3);
        for (size_t v = 0; v < xyz.size() / 3; ++v) std::printf("%.9g %.9g %.9g\n", xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2]);
        for (size_t t = 0; t < tris.size() / 3; ++t) std::printf("%d %d %d\n", tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]);
    }
    return 0;
}
