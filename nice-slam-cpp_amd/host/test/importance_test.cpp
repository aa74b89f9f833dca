// importance_test.cpp -- Renderer::render_batch_ray with rendering.N_importance from the command line, and its driver for
// tests/test_gpu_importance.py.
//   importance_test <dir> <stage> <N_importance>
//        the scene in <dir> (bound.npy [3,2], grid_{coarse,middle,fine,color}.npy [1,32,Z,Y,X], dec_{coarse,middle,fine,color}.npy packed),
//        the rays rays_o.npy / rays_d.npy [N,3] and, optionally, their depths gt_depth.npy [N]
//        -> <dir>/imp_rgb.npy [N,3], imp_depth.npy [N], imp_var.npy [N], imp_weights.npy [N, N_samples (+ N_surface) + N_importance] (float32)
//        N_importance reaches the Renderer as the key rendering.N_importance of a configuration node, as it does from a file
//   importance_test --config <nice_slam.yaml> <cofusion.yaml>
//        the N_importance of a Renderer, a Tracker and a Mapper built from the two files, one JSON line (no device): tests/test_importance_cpu.py
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "Mapper.h"
#include "Renderer.h"
#include "Tracker.h"

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

// what the Renderer, a Tracker and a Mapper built from the two configuration files carry as N_importance: one JSON line, no device
static int print_config(const std::string& ns_path, const std::string& cf_path)
{
    YAML::Node ns = YAML::LoadFile(ns_path), cf = YAML::LoadFile(cf_path);
    Renderer renderer(ns);
    Tracker tracker(ns, cf, c10::Dict<std::string, torch::Tensor>());
    Mapper mapper(ns, cf, false);
    std::printf("{\"renderer\": %d, \"tracker\": %d, \"mapper\": %d}\n", renderer.N_importance, tracker.n_importance(), mapper.n_importance());
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: importance_test <dir> <stage> <N_importance> | importance_test --config <nice_slam.yaml> <cofusion.yaml>\n"); return 2; }
    try {
        if (std::string(argv[1]) == "--config") return print_config(argv[2], argv[3]);
        const std::string dir = std::string(argv[1]) + "/", stage = argv[2];
        c10::Dict<std::string, torch::Tensor> c;
        for (auto k : {"grid_coarse", "grid_middle", "grid_fine", "grid_color"}) c.insert(k, load_npy(dir + k + ".npy"));
        NICE decoders(3, 32, 32, 2.f, 0.32f, 0.16f, 0.16f, true, "fourier");
        decoders.coarse_decoder->unpack(load_npy(dir + "dec_coarse.npy"));
        decoders.middle_decoder->unpack(load_npy(dir + "dec_middle.npy"));
        decoders.fine_decoder->unpack(load_npy(dir + "dec_fine.npy"));
        decoders.color_decoder->unpack(load_npy(dir + "dec_color.npy"));
        std::istringstream ns_s(std::string("rendering:\n  N_importance: ") + argv[3] + "\n");      // the value travels as the configuration's key
        Renderer renderer(YAML::Load(ns_s));
        renderer.set_bound(load_npy(dir + "bound.npy"));
        torch::Tensor gt_depth;
        if (exists(dir + "gt_depth.npy")) gt_depth = load_npy(dir + "gt_depth.npy");
        torch::Tensor rgb, depth, var, weights;
        renderer.render_batch_ray(c, decoders, load_npy(dir + "rays_d.npy"), load_npy(dir + "rays_o.npy"), stage, gt_depth, rgb, depth, var, weights);
        save_npy(dir + "imp_rgb.npy", rgb);
        save_npy(dir + "imp_depth.npy", depth);
        save_npy(dir + "imp_var.npy", var);
        save_npy(dir + "imp_weights.npy", weights);
        std::printf("importance_test ok: %d rays x %d samples, stage %s, N_importance %d, %s depths\n", (int)depth.size(0), (int)weights.size(1),
                    stage.c_str(), renderer.N_importance, gt_depth.defined() ? "with" : "no");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "importance_test failed: %s\n", e.what());
        return 1;
    }
}
