// mesh_test.cpp -- driver of the Mesher for tests/test_mesh_cpu.py and tests/test_gpu_mesh.py.
//   mesh_test ply <file.ply> <color 0|1>        write a small fixed mesh, read it back, compare (no GPU)
//   mesh_test scene <dir> <resolution> <color 0|1> [padding [simplify_cell]]
//        the scene in <dir> (bound.npy [3,2], grid_{coarse,middle,fine,color}.npy [1,32,Z,Y,X], dec_{coarse,middle,fine,color}.npy packed,
//        optional valid.npy [resolution^3] as float 0 / 1) through Mesher::get_mesh -> <dir>/mesh.ply; simplify_cell given: the member is set
//        to it (0 included), else it is never touched
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

static bool exists(const std::string& p) { std::ifstream f(p); return (bool)f; }

int main(int argc, char** argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: mesh_test ply <file> <color> | mesh_test scene <dir> <resolution> <color> [padding]\n"); return 2; }
    const std::string mode = argv[1];
    try {
        if (mode == "ply") {
            const bool color = std::atoi(argv[3]) != 0;
            const int n = 7;
            std::vector<float> xyz; std::vector<uint8_t> rgb; std::vector<int32_t> tris;
            for (int k = 0; k < n; ++k) {
                xyz.push_back(0.5f * k); xyz.push_back((float)(k * k)); xyz.push_back(-(float)k);
                rgb.push_back((uint8_t)(30 * k)); rgb.push_back((uint8_t)(255 - k)); rgb.push_back(7);
            }
            for (int t = 0; t < 5; ++t) { tris.push_back(t); tris.push_back(t + 1); tris.push_back(t + 2); }
            Mesher::write_ply(argv[2], xyz.data(), color ? rgb.data() : nullptr, n, tris.data(), 5);
            std::vector<float> xyz2; std::vector<uint8_t> rgb2; std::vector<int32_t> tris2;
            Mesher::read_ply(argv[2], xyz2, rgb2, tris2);
            if (xyz2 != xyz || tris2 != tris || (color ? rgb2 != rgb : !rgb2.empty())) { std::fprintf(stderr, "PLY round trip differs\n"); return 1; }
            std::printf("mesh_test ply ok\n");
            return 0;
        }
        if (mode != "scene" || argc < 5) { std::fprintf(stderr, "unknown mode\n"); return 2; }
        const std::string dir = std::string(argv[2]) + "/";
        std::ostringstream y;
        y << "meshing:\n  level_set: 0\n  resolution: " << std::atoi(argv[3]) << "\n";
        std::istringstream ys(y.str());
        YAML::Node ns = YAML::Load(ys);
        c10::Dict<std::string, torch::Tensor> c;
        for (auto k : {"grid_coarse", "grid_middle", "grid_fine", "grid_color"}) c.insert(k, load_npy(dir + k + ".npy"));
        NICE decoders(3, 32, 32, 2.f, 0.32f, 0.16f, 0.16f, true, "fourier");
        decoders.coarse_decoder->unpack(load_npy(dir + "dec_coarse.npy"));
        decoders.middle_decoder->unpack(load_npy(dir + "dec_middle.npy"));
        decoders.fine_decoder->unpack(load_npy(dir + "dec_fine.npy"));
        decoders.color_decoder->unpack(load_npy(dir + "dec_color.npy"));
        Mesher mesher(ns, load_npy(dir + "bound.npy"), argc > 5 ? (float)std::atof(argv[5]) : 0.f);
        torch::Tensor valid;
        if (exists(dir + "valid.npy")) valid = load_npy(dir + "valid.npy").ne(0).to(torch::kUInt8);
        if (argc > 6) mesher.simplify_cell = (float)std::atof(argv[6]);
        mesher.get_mesh(dir + "mesh.ply", decoders, c, std::atoi(argv[4]) != 0, valid);
        std::printf("mesh_test scene ok: %d vertices, %d triangles\n", mesher.last_vertices, mesher.last_triangles);
        if (argc > 6) std::printf("simplified: %d vertices, %d triangles, %d collapsed, %d duplicates\n", mesher.last_simplified_vertices,
                                  mesher.last_simplified_triangles, mesher.last_collapsed, mesher.last_duplicates);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "mesh_test failed: %s\n", e.what());
        return 1;
    }
}
