// eval_img_test A.npy B.npy [levels] [data_range] -- Renderer::image_ssim on two images ([H][W] or [H][W][C] float32 .npy files), one JSON
// line (tests/test_gpu_ssim.py); levels 1: SSIM, 5: MS-SSIM with the standard weights
#include <cstdio>
#include <cstdlib>
#include <exception>
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

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s A.npy B.npy [levels] [data_range]\n", argv[0]); return 2; }
    const int levels = argc > 3 ? std::atoi(argv[3]) : 1;
    const double data_range = argc > 4 ? std::atof(argv[4]) : 1.0;
    try {
        Renderer renderer;
        double h[8];
        const std::pair<double, double> r = renderer.image_ssim(load_npy(argv[1]), load_npy(argv[2]), levels, data_range, h);
        std::printf("{\"ssim\": %.17g, \"ms_ssim\": ", r.second);
        if (levels > 1) std::printf("%.17g", r.first); else std::printf("null");
        std::printf(", \"left_out\": %lld, \"Hm\": %d, \"Wm\": %d, \"levels\": %d, \"data_range\": %.17g}\n", (long long)h[3], (int)h[5], (int)h[6], levels, data_range);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "eval_img_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
