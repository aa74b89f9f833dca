// clean_mesh_test.cpp -- driver of Mesher::get_clean_mesh for tests/test_gpu_mesh_cull.py.
//   clean_mesh_test <dir> <resolution> <color 0|1> <padding> <min_area> <largest 0|1>
//        the scene in <dir> (bound.npy [3,2], grid_{coarse,middle,fine,color}.npy [1,32,Z,Y,X], dec_{coarse,middle,fine,color}.npy packed), the
//        keyframes depths.npy [K,H,W] and c2ws.npy [K,4,4], intr.npy [4] = fx, fy, cx, cy  ->  <dir>/clean_mesh.ply
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

int main(int argc, char** argv)
{
    if (argc < 7) { std::fprintf(stderr, "usage: clean_mesh_test <dir> <resolution> <color> <padding> <min_area> <largest>\n"); return 2; }
    try {
        const std::string dir = std::string(argv[1]) + "/";
        std::ostringstream y;
        y << "meshing:\n  level_set: 0\n  resolution: " << std::atoi(argv[2]) << "\n  remove_small_geometry_threshold: " << argv[5]
          << "\n  get_largest_components: " << (std::atoi(argv[6]) ? "True" : "False") << "\n";
        std::istringstream ys(y.str());
        YAML::Node ns = YAML::Load(ys);
        c10::Dict<std::string, torch::Tensor> c;
        for (auto k : {"grid_coarse", "grid_middle", "grid_fine", "grid_color"}) c.insert(k, load_npy(dir + k + ".npy"));
        NICE decoders(3, 32, 32, 2.f, 0.32f, 0.16f, 0.16f, true, "fourier");
        decoders.coarse_decoder->unpack(load_npy(dir + "dec_coarse.npy"));
        decoders.middle_decoder->unpack(load_npy(dir + "dec_middle.npy"));
        decoders.fine_decoder->unpack(load_npy(dir + "dec_fine.npy"));
        decoders.color_decoder->unpack(load_npy(dir + "dec_color.npy"));
        Mesher mesher(ns, load_npy(dir + "bound.npy"), (float)std::atof(argv[4]));
        torch::Tensor depths = load_npy(dir + "depths.npy"), c2ws = load_npy(dir + "c2ws.npy"), intr = load_npy(dir + "intr.npy");
        if (depths.dim() != 3 || c2ws.dim() != 3 || depths.size(0) != c2ws.size(0) || intr.numel() != 4) throw std::runtime_error("depths [K,H,W], c2ws [K,4,4], intr [4] expected");
        std::vector<torch::Tensor> dv, cv;
        for (int64_t k = 0; k < depths.size(0); ++k) { dv.push_back(depths[k]); cv.push_back(c2ws[k]); }
        const float* in = intr.data_ptr<float>();
        mesher.get_clean_mesh(dir + "clean_mesh.ply", decoders, c, dv, cv, (int)depths.size(1), (int)depths.size(2), in[0], in[1], in[2], in[3], std::atoi(argv[3]) != 0);
        std::printf("clean_mesh_test ok: %d vertices, %d triangles, %d components, %d kept, %lld seen, %lld evaluated of %lld nodes\n", mesher.last_vertices,
                    mesher.last_triangles, mesher.last_components, mesher.last_kept, mesher.last_seen, mesher.last_evaluated,
                    (long long)mesher.resolution * mesher.resolution * mesher.resolution);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "clean_mesh_test failed: %s\n", e.what());
        return 1;
    }
}
