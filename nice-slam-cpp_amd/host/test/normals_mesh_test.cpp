// normals_mesh_test.cpp -- driver of the Mesher's vertex normals and colouring methods for tests/test_normals_cpu.py and tests/test_gpu_normals.py.
//   normals_mesh_test <dir> <out.ply> <resolution> <method> <length> <write_normals 0|1> [padding]
//        the scene in <dir> (bound.npy [3,2], grid_{coarse,middle,fine,color}.npy [1,32,Z,Y,X], dec_{coarse,middle,fine,color}.npy packed)
//        through Mesher::get_mesh with meshing.color_mesh_extraction_method = <method>, color_ray_length = <length> -> <out.ply>, one JSON line
//   normals_mesh_test ply <dir>       (no GPU) xyz.npy / normals.npy [n,3], rgb.npy [n,3] (0 .. 255), tris.npy [m,3], all float32, in <dir> ->
//        with_normals.ply (the new write_ply), old.ply (the old write_ply), no_normals.ply (the new one without normals); every reader on them
//   normals_mesh_test config <method | ->     (no GPU) the Mesher's color_method for that value of the key (-: the key is absent)
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

template <class T> static bool same(const std::vector<T>& a, const std::vector<T>& b)          // the bytes (a NaN equals itself)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static YAML::Node config(int resolution, const std::string& method)
{
    std::ostringstream y;
    y << "meshing:\n  level_set: 0\n  resolution: " << resolution << "\n";
    if (method != "-") y << "  color_mesh_extraction_method: " << method << "\n";
    std::istringstream ys(y.str());
    return YAML::Load(ys);
}

static int ply_mode(const std::string& dir)
{
    const torch::Tensor X = load_npy(dir + "xyz.npy"), Nn = load_npy(dir + "normals.npy"), C = load_npy(dir + "rgb.npy"), T = load_npy(dir + "tris.npy");
    const int nv = (int)X.size(0), nt = (int)T.size(0);
    std::vector<float> xyz(X.data_ptr<float>(), X.data_ptr<float>() + 3 * (size_t)nv), nrm(Nn.data_ptr<float>(), Nn.data_ptr<float>() + 3 * (size_t)nv);
    std::vector<uint8_t> rgb(3 * (size_t)nv);
    std::vector<int32_t> tris(3 * (size_t)nt);
    for (size_t k = 0; k < rgb.size(); ++k) rgb[k] = (uint8_t)C.data_ptr<float>()[k];
    for (size_t k = 0; k < tris.size(); ++k) tris[k] = (int32_t)T.data_ptr<float>()[k];
    Mesher::write_ply(dir + "with_normals.ply", xyz.data(), nrm.data(), rgb.data(), nv, tris.data(), nt);
    Mesher::write_ply(dir + "normals_only.ply", xyz.data(), nrm.data(), nullptr, nv, tris.data(), nt);
    Mesher::write_ply(dir + "old.ply", xyz.data(), rgb.data(), nv, tris.data(), nt);
    Mesher::write_ply(dir + "no_normals.ply", xyz.data(), nullptr, rgb.data(), nv, tris.data(), nt);
    std::vector<float> x2, n2; std::vector<uint8_t> c2; std::vector<int32_t> t2;
    Mesher::read_ply(dir + "with_normals.ply", x2, n2, c2, t2);
    if (!same(x2, xyz) || !same(n2, nrm) || !same(c2, rgb) || !same(t2, tris)) { std::fprintf(stderr, "with_normals.ply: the round trip differs\n"); return 1; }
    Mesher::read_ply(dir + "normals_only.ply", x2, n2, c2, t2);
    if (!same(x2, xyz) || !same(n2, nrm) || !c2.empty() || !same(t2, tris)) { std::fprintf(stderr, "normals_only.ply: the round trip differs\n"); return 1; }
    Mesher::read_ply(dir + "old.ply", x2, n2, c2, t2);      // the new reader on a file without normals
    if (!same(x2, xyz) || !n2.empty() || !same(c2, rgb) || !same(t2, tris)) { std::fprintf(stderr, "old.ply: the new reader differs\n"); return 1; }
    Mesher::read_ply(dir + "old.ply", x2, c2, t2);          // the old reader
    if (!same(x2, xyz) || !same(c2, rgb) || !same(t2, tris)) { std::fprintf(stderr, "old.ply: the old reader differs\n"); return 1; }
    Mesher::read_ply_mesh(dir + "with_normals.ply", x2, t2);        // the general reader skips nx ny nz and the colours
    if (!same(x2, xyz) || !same(t2, tris)) { std::fprintf(stderr, "with_normals.ply: read_ply_mesh differs\n"); return 1; }
    bool threw = false;
    try { Mesher::read_ply(dir + "with_normals.ply", x2, c2, t2); } catch (const std::runtime_error&) { threw = true; }     // as before: not its file
    if (!threw) { std::fprintf(stderr, "the old reader took a file with normals\n"); return 1; }
    std::printf("normals_mesh_test ply ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    const char* usage = "usage: normals_mesh_test <dir> <out.ply> <resolution> <method> <length> <write_normals> [padding] | ply <dir> | config <method | ->\n";
    if (argc < 3) { std::fprintf(stderr, "%s", usage); return 2; }
    try {
        if (std::string(argv[1]) == "ply" && argc == 3) return ply_mode(std::string(argv[2]) + "/");
        if (std::string(argv[1]) == "config" && argc == 3) {
            Mesher mesher(config(8, argv[2]));
            std::printf("{\"color_method\": \"%s\", \"color_ray_length\": %.9g, \"write_normals\": %d}\n", mesher.color_method.c_str(),
                        (double)mesher.color_ray_length, mesher.write_normals ? 1 : 0);
            return 0;
        }
        if (argc < 7) { std::fprintf(stderr, "%s", usage); return 2; }
        const std::string dir = std::string(argv[1]) + "/";
        c10::Dict<std::string, torch::Tensor> c;
        for (auto k : {"grid_coarse", "grid_middle", "grid_fine", "grid_color"}) c.insert(k, load_npy(dir + k + ".npy"));
        NICE decoders(3, 32, 32, 2.f, 0.32f, 0.16f, 0.16f, true, "fourier");
        decoders.coarse_decoder->unpack(load_npy(dir + "dec_coarse.npy"));
        decoders.middle_decoder->unpack(load_npy(dir + "dec_middle.npy"));
        decoders.fine_decoder->unpack(load_npy(dir + "dec_fine.npy"));
        decoders.color_decoder->unpack(load_npy(dir + "dec_color.npy"));
        Mesher mesher(config(std::atoi(argv[3]), argv[4]), load_npy(dir + "bound.npy"), argc > 7 ? (float)std::atof(argv[7]) : 0.f);
        mesher.color_ray_length = (float)std::atof(argv[5]);
        mesher.write_normals = std::atoi(argv[6]) != 0;
        mesher.get_mesh(argv[2], decoders, c, true);
        std::printf("{\"vertices\": %d, \"triangles\": %d, \"fallback\": %d, \"without_normal\": %d, \"method\": \"%s\"}\n", mesher.last_vertices,
                    mesher.last_triangles, mesher.last_color_fallback, mesher.last_normals_zero, mesher.color_method.c_str());
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "normals_mesh_test failed: %s\n", e.what());
        return 1;
    }
}
