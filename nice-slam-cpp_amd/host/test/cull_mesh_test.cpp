// cull_mesh_test.cpp -- driver of Mesher::cull_mesh for tests/test_gpu_cull.py.
//   cull_mesh_test DIR IN.ply OUT.ply none|depth|self EDGE EPS [UNSEEN_N UNSEEN.npy]
//        the trajectory in DIR, in clean_mesh_test's layout: c2ws.npy [K,4,4] camera-to-world (inverted here in double, rounded once),
//        intr.npy [4] = fx, fy, cx, cy, depths.npy [K,H,W] (read for H and W in every mode, for its values with `depth`)
//        ->  OUT.ply: the part of IN.ply the trajectory saw;  UNSEEN.npy [UNSEEN_N,3] float32: samples of the part it did not see
//        (Mesher::unseen_points, seed 0);  one JSON line on stdout
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "Mesher.h"

static torch::Tensor load_npy(const std::string& path)       // little-endian float32, C order (what numpy.save writes for such an array)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    char magic[8];
    f.read(magic, 8);
    size_t hl = 0;
    if (magic[6] == 1) { uint16_t v; f.read((char*)&v, 2); hl = v; } else { uint32_t v; f.read((char*)&v, 4); hl = v; }
    std::string hdr(hl, ' ');
    f.read(&hdr[0], (std::streamsize)hl);
    if (hdr.find("'<f4'") == std::string::npos || hdr.find("'fortran_order': False") == std::string::npos) throw std::runtime_error(path + ": float32 C-order expected");
    const size_t a = hdr.find('(', hdr.find("'shape'")), b = hdr.find(')', a);
    std::vector<int64_t> shape;
    std::istringstream ss(hdr.substr(a + 1, b - a - 1));
    std::string tok;
    while (std::getline(ss, tok, ',')) { if (tok.find_first_of("0123456789") != std::string::npos) shape.push_back(std::stoll(tok)); }
    torch::Tensor t = torch::empty(shape, torch::kFloat32);
    f.read((char*)t.data_ptr<float>(), (std::streamsize)(t.numel() * sizeof(float)));
    if (!f) throw std::runtime_error(path + ": truncated");
    return t;
}

static void save_npy_n3(const std::string& path, const std::vector<float>& xyz)      // float32 [n, 3], format version 1.0
{
    std::string hdr = "{'descr': '<f4', 'fortran_order': False, 'shape': (" + std::to_string(xyz.size() / 3) + ", 3), }";
    while ((10 + hdr.size() + 1) % 64 != 0) hdr += ' ';
    hdr += '\n';
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot write " + path);
    const uint16_t hl = (uint16_t)hdr.size();
    f.write("\x93NUMPY\x01\x00", 8);
    f.write((const char*)&hl, 2);
    f.write(hdr.data(), (std::streamsize)hdr.size());
    f.write((const char*)xyz.data(), (std::streamsize)(xyz.size() * sizeof(float)));
    if (!f) throw std::runtime_error(path + ": write failed");
}

int main(int argc, char** argv)
{
    if (argc != 7 && argc != 9) { std::fprintf(stderr, "usage: cull_mesh_test DIR IN.ply OUT.ply none|depth|self EDGE EPS [UNSEEN_N UNSEEN.npy]\n"); return 2; }
    try {
        const std::string dir = std::string(argv[1]) + "/", occlusion = argv[4];
        const int edge = std::atoi(argv[5]);
        const float eps = (float)std::atof(argv[6]);
        torch::Tensor depths = load_npy(dir + "depths.npy"), c2ws = load_npy(dir + "c2ws.npy"), intr = load_npy(dir + "intr.npy");
        if (depths.dim() != 3 || c2ws.dim() != 3 || depths.size(0) != c2ws.size(0) || intr.numel() != 4) throw std::runtime_error("depths [K,H,W], c2ws [K,4,4], intr [4] expected");
        const int K = (int)depths.size(0), H = (int)depths.size(1), W = (int)depths.size(2);
        std::vector<float> w2c((size_t)K * 16);
        for (int k = 0; k < K; ++k) {
            torch::Tensor inv = torch::linalg_inv(c2ws[k].to(torch::kFloat64).view({4, 4})).to(torch::kFloat32).contiguous();      // inverted in double, rounded once
            std::memcpy(&w2c[(size_t)k * 16], inv.data_ptr<float>(), 16 * sizeof(float));
        }
        const float* in = intr.data_ptr<float>();
        std::vector<float> xyz;
        std::vector<int32_t> tris;
        Mesher::read_ply_mesh(argv[2], xyz, tris);
        const int nv = (int)(xyz.size() / 3), nt = (int)(tris.size() / 3);
        const CulledMesh R = Mesher::cull_mesh(xyz.data(), nv, tris.data(), nt, w2c.data(), K, H, W, in[0], in[1], in[2], in[3],
                                               depths.data_ptr<float>(), occlusion, edge, eps);
        Mesher::write_ply(argv[3], R.xyz.data(), nullptr, (int)(R.xyz.size() / 3), R.triangles.data(), (int)(R.triangles.size() / 3));
        long long n_unseen = -1;
        if (argc == 9) {
            const std::vector<float> u = Mesher::unseen_points(xyz.data(), nv, tris.data(), nt, R.seen.data(), std::atoi(argv[7]), 0ull);
            save_npy_n3(argv[8], u);
            n_unseen = (long long)(u.size() / 3);
        }
        std::printf("{\"occlusion\": \"%s\", \"frames\": %d, \"H\": %d, \"W\": %d, \"in_vertices\": %d, \"in_triangles\": %d, \"vertices\": %d, "
                    "\"triangles\": %d, \"n_seen\": %lld, \"skipped\": %d, \"unseen_points\": %lld}\n", occlusion.c_str(), K, H, W, nv, nt,
                    (int)(R.xyz.size() / 3), (int)(R.triangles.size() / 3), R.n_seen, R.skipped, n_unseen);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "cull_mesh_test failed: %s\n", e.what());
        return 1;
    }
}
