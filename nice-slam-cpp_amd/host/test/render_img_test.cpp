// render_img_test.cpp -- Renderer::render_img from the command line, and its driver for tests/test_gpu_render_image.py.
//   render_img_test <dir> <stage> <H> <W> <fx> <fy> <cx> <cy>
//        the scene in <dir> (bound.npy [3,2], grid_{coarse,middle,fine,color}.npy [1,32,Z,Y,X], dec_{coarse,middle,fine,color}.npy packed),
//        the pose c2w.npy [3,4] or [4,4] and, optionally, the depth image depth.npy [H,W]
//        -> <dir>/img_depth.npy [H,W], img_var.npy [H,W], img_rgb.npy [H,W,3] (float32)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "Renderer.h"

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

static void save_npy(const std::string& path, const torch::Tensor& t)       // float32, C order, format version 1.0
{
    torch::Tensor h = t.detach().to(torch::kCPU, torch::kFloat32).contiguous();
    std::ostringstream d;
    d << "{'descr': '<f4', 'fortran_order': False, 'shape': (";
    for (int64_t k = 0; k < h.dim(); ++k) d << h.size(k) << (h.dim() == 1 || k + 1 < h.dim() ? "," : "") << (k + 1 < h.dim() ? " " : "");
    d << "), }";
    std::string hdr = d.str();
    while ((10 + hdr.size() + 1) % 64 != 0) hdr.push_back(' ');
    hdr.push_back('\n');
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot write " + path);
    const uint16_t hl = (uint16_t)hdr.size();
    f.write("\x93NUMPY\x01\x00", 8);
    f.write((const char*)&hl, 2);
    f.write(hdr.data(), (std::streamsize)hdr.size());
    f.write((const char*)h.data_ptr<float>(), (std::streamsize)(h.numel() * sizeof(float)));
    if (!f) throw std::runtime_error(path + ": write failed");
}

static bool exists(const std::string& p) { std::ifstream f(p); return (bool)f; }

int main(int argc, char** argv)
{
    if (argc < 9) { std::fprintf(stderr, "usage: render_img_test <dir> <stage> <H> <W> <fx> <fy> <cx> <cy>\n"); return 2; }
    try {
        const std::string dir = std::string(argv[1]) + "/", stage = argv[2];
        const int H = std::atoi(argv[3]), W = std::atoi(argv[4]);
        const float fx = (float)std::atof(argv[5]), fy = (float)std::atof(argv[6]), cx = (float)std::atof(argv[7]), cy = (float)std::atof(argv[8]);
        c10::Dict<std::string, torch::Tensor> c;
        for (auto k : {"grid_coarse", "grid_middle", "grid_fine", "grid_color"}) c.insert(k, load_npy(dir + k + ".npy"));
        NICE decoders(3, 32, 32, 2.f, 0.32f, 0.16f, 0.16f, true, "fourier");
        decoders.coarse_decoder->unpack(load_npy(dir + "dec_coarse.npy"));
        decoders.middle_decoder->unpack(load_npy(dir + "dec_middle.npy"));
        decoders.fine_decoder->unpack(load_npy(dir + "dec_fine.npy"));
        decoders.color_decoder->unpack(load_npy(dir + "dec_color.npy"));
        Renderer renderer;
        renderer.set_bound(load_npy(dir + "bound.npy"));
        torch::Tensor gt_depth;
        if (exists(dir + "depth.npy")) gt_depth = load_npy(dir + "depth.npy");
        torch::Tensor depth, var, rgb;
        std::tie(depth, var, rgb) = renderer.render_img(c, decoders, load_npy(dir + "c2w.npy"), stage, gt_depth, H, W, fx, fy, cx, cy);
        save_npy(dir + "img_depth.npy", depth);
        save_npy(dir + "img_var.npy", var);
        save_npy(dir + "img_rgb.npy", rgb);
        std::printf("render_img_test ok: %d x %d, stage %s, %s depth image\n", H, W, stage.c_str(), gt_depth.defined() ? "with a" : "no");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "render_img_test failed: %s\n", e.what());
        return 1;
    }
}
