// hull_mesh_test.cpp -- driver of Mesher::get_hull_mesh for tests/test_gpu_hull_mesh.py.
//   hull_mesh_test DIR OUT.ply RES [SCALE]
//        the trajectory in DIR, in fuse_mesh_test's layout: c2ws.npy [K,4,4] camera-to-world (inverted in double, rounded once), intr.npy [4]
//        = fx, fy, cx, cy, depths.npy [K,H,W]; bound.npy [3,2]: the lattice has RES nodes per axis over it (no padding, no component filter);
//        the scene in clean_mesh_test's layout (grid_*.npy, dec_*.npy).  SCALE: meshing.clean_mesh_bound_scale; left out, the key is absent
//        from the configuration and the Mesher's default holds.  With hull_xyz.npy [V,3] and hull_faces.npy [F,3] (vertex numbers as
//        float32) in DIR that mesh is uploaded as the bound (nsk_hull_upload) and the frames are not fused.
//        ->  OUT.ply: the map's mesh inside the scaled hull, without colours;  one JSON line on stdout
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "Mesher.h"
#include "nsk_devarr.h"

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
    if (argc != 4 && argc != 5) { std::fprintf(stderr, "usage: hull_mesh_test DIR OUT.ply RES [SCALE]\n"); return 2; }
    try {
        const std::string dir = std::string(argv[1]) + "/";
        std::ostringstream y;
        y << "meshing:\n  level_set: 0\n  resolution: " << std::atoi(argv[3]) << "\n  remove_small_geometry_threshold: 0\n  get_largest_components: False\n";
        if (argc == 5) y << "  clean_mesh_bound_scale: " << argv[4] << "\n";
        std::istringstream ys(y.str());
        YAML::Node ns = YAML::Load(ys);
        Mesher mesher(ns, load_npy(dir + "bound.npy"), 0.f);
        torch::Tensor depths = load_npy(dir + "depths.npy"), c2ws = load_npy(dir + "c2ws.npy"), intr = load_npy(dir + "intr.npy");
        if (depths.dim() != 3 || c2ws.dim() != 3 || depths.size(0) != c2ws.size(0) || intr.numel() != 4) throw std::runtime_error("depths [K,H,W], c2ws [K,4,4], intr [4] expected");
        const int K = (int)depths.size(0), H = (int)depths.size(1), W = (int)depths.size(2);
        std::vector<torch::Tensor> dv, cv;
        for (int64_t k = 0; k < K; ++k) { dv.push_back(depths[k]); cv.push_back(c2ws[k]); }
        const float* in = intr.data_ptr<float>();
        c10::Dict<std::string, torch::Tensor> c;
        for (auto k : {"grid_coarse", "grid_middle", "grid_fine", "grid_color"}) c.insert(k, load_npy(dir + k + ".npy"));
        NICE decoders(3, 32, 32, 2.f, 0.32f, 0.16f, 0.16f, true, "fourier");
        decoders.coarse_decoder->unpack(load_npy(dir + "dec_coarse.npy"));
        decoders.middle_decoder->unpack(load_npy(dir + "dec_middle.npy"));
        decoders.fine_decoder->unpack(load_npy(dir + "dec_fine.npy"));
        decoders.color_decoder->unpack(load_npy(dir + "dec_color.npy"));
        if (std::ifstream(dir + "hull_xyz.npy").good()) {
            torch::Tensor xyz = load_npy(dir + "hull_xyz.npy").contiguous(), faces = load_npy(dir + "hull_faces.npy").to(torch::kInt32).contiguous();
            nskh::check(nsk_hull_upload(nskh::ctx(), xyz.data_ptr<float>(), (int)xyz.size(0), faces.data_ptr<int32_t>(), (int)faces.size(0)));
            mesher.hull_from_context = true;
        }
        mesher.get_hull_mesh(argv[2], decoders, c, dv, cv, H, W, in[0], in[1], in[2], in[3], false);
        std::printf("{\"frames\": %d, \"H\": %d, \"W\": %d, \"resolution\": %d, \"scale\": %.9g, \"uploaded\": %d, \"n_observed\": %lld, \"hull_vertices\": %zu, "
                    "\"hull_faces\": %zu, \"inside\": %lld, \"evaluated\": %lld, \"vertices\": %d, \"triangles\": %d}\n", K, H, W, mesher.resolution,
                    (double)mesher.clean_mesh_bound_scale, mesher.hull_from_context ? 1 : 0, mesher.last_observed, mesher.last_hull_vertices.size(),
                    mesher.last_hull_faces.size() / 3, mesher.last_inside, mesher.last_evaluated, mesher.last_vertices, mesher.last_triangles);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "hull_mesh_test failed: %s\n", e.what());
        return 1;
    }
}
