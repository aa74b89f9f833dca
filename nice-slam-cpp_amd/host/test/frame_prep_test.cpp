// frame_prep_test.cpp -- nskh::FramePrep from the command line, and its driver for tests/test_gpu_frame.py.
//   frame_prep_test <dir> <cam.yaml>
//        <dir>/color.npy [H,W,3] uint8 and <dir>/depth.npy [H,W] uint16, one raw frame; the YAML file's cam block (H W fx fy cx cy, optional
//        crop_edge, crop_size: [H, W], distortion: [...], png_depth_scale, scale)
//        -> <dir>/prep_color.npy [H',W',3], <dir>/prep_depth.npy [H',W'] (float32) and one JSON line: H W fx fy cx cy n_border
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "FramePrep.h"

// little-endian C-order array of the given descr (what numpy.save writes): the bytes and the shape
static std::vector<unsigned char> load_npy(const std::string& path, const std::string& descr, size_t item, std::vector<int64_t>& shape)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    char magic[8];
    f.read(magic, 8);
    size_t hl = 0;
    if (magic[6] == 1) { uint16_t v; f.read((char*)&v, 2); hl = v; } else { uint32_t v; f.read((char*)&v, 4); hl = v; }
    std::string hdr(hl, ' ');
    f.read(&hdr[0], (std::streamsize)hl);
    if (hdr.find("'" + descr + "'") == std::string::npos || hdr.find("'fortran_order': False") == std::string::npos) throw std::runtime_error(path + ": " + descr + " C-order expected");
    const size_t a = hdr.find('(', hdr.find("'shape'")), b = hdr.find(')', a);
    std::istringstream ss(hdr.substr(a + 1, b - a - 1));
    std::string tok;
    size_t n = 1;
    shape.clear();
    while (std::getline(ss, tok, ',')) { if (tok.find_first_of("0123456789") != std::string::npos) { shape.push_back(std::stoll(tok)); n *= (size_t)shape.back(); } }
    std::vector<unsigned char> data(n * item);
    f.read((char*)data.data(), (std::streamsize)data.size());
    if (!f) throw std::runtime_error(path + ": truncated");
    return data;
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

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: frame_prep_test <dir> <cam.yaml>\n"); return 2; }
    const std::string dir = std::string(argv[1]) + "/";
    try {
        YAML::Node cfg = YAML::LoadFile(argv[2]);
        nskh::FramePrep prep(cfg["cam"]);
        std::vector<int64_t> cs, ds;
        std::vector<unsigned char> color = load_npy(dir + "color.npy", "|u1", 1, cs), depth = load_npy(dir + "depth.npy", "<u2", 2, ds);
        if (cs.size() != 3 || cs[2] != 3 || ds.size() != 2) throw std::runtime_error("color.npy must be [H,W,3], depth.npy [H,W]");
        cv::Mat raw_rgb((int)cs[0], (int)cs[1], CV_8UC3, color.data()), raw_depth((int)ds[0], (int)ds[1], CV_16UC1, depth.data());
        auto out = prep.prepare(raw_rgb, raw_depth);
        save_npy(dir + "prep_color.npy", out.first);
        save_npy(dir + "prep_depth.npy", out.second);
        std::printf("{\"H\": %d, \"W\": %d, \"fx\": %.9g, \"fy\": %.9g, \"cx\": %.9g, \"cy\": %.9g, \"n_border\": %d}\n", prep.H, prep.W, (double)prep.fx,
                    (double)prep.fy, (double)prep.cx, (double)prep.cy, prep.last_border);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "frame_prep_test failed: %s\n", e.what());
        return 1;
    }
}
