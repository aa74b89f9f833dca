// nsk_mesher.cpp -- Mesher (include/Mesher.h): lattice evaluation and marching cubes stay on the device; the host writes the PLY.
#include "Mesher.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include <hip/hip_runtime_api.h>

#include "nsk_host.h"

using nskh::check;
using nskh::ctx;

Mesher::Mesher(YAML::Node ns, torch::Tensor bound_3x2, float padding_) : padding(padding_)
{
    resolution = ns["meshing"]["resolution"].IsDefined() ? ns["meshing"]["resolution"].as<int>() : 256;
    level_set = ns["meshing"]["level_set"].IsDefined() ? ns["meshing"]["level_set"].as<float>() : 0.f;
    remove_small_geometry_threshold = ns["meshing"]["remove_small_geometry_threshold"].IsDefined() ? ns["meshing"]["remove_small_geometry_threshold"].as<float>() : 0.2f;
    get_largest_components = ns["meshing"]["get_largest_components"].IsDefined() ? ns["meshing"]["get_largest_components"].as<bool>() : false;
    if (resolution < 2) throw std::runtime_error("Mesher: meshing.resolution must be at least 2");
    if (!(padding >= 0.f)) throw std::runtime_error("Mesher: padding must be >= 0");
    bound = bound_3x2.defined() ? bound_3x2.detach().to(torch::kCPU, torch::kFloat32).contiguous().clone()
                                : torch::tensor({{-4.5f, 3.82f}, {-1.5f, 2.02f}, {-3.0f, 2.76f}});      // src/Renderer.cpp:15
}

void Mesher::set_bound(torch::Tensor b) { bound = b.detach().to(torch::kCPU, torch::kFloat32).contiguous().clone(); }

namespace {
struct DevMem {
    void* p = nullptr;
    explicit DevMem(size_t bytes) { if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) throw std::runtime_error("Mesher: hipMalloc of " + std::to_string(bytes) + " bytes failed"); }
    ~DevMem() { if (p) hipFree(p); }
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
};
}  // namespace

// the context's mesh (nv vertices, nt triangles) -> host, the colour query on the device vertex buffer, the PLY
static void write_context_mesh(const std::string& path, bool color, int nv, int nt)
{
    std::vector<float> xyz((size_t)nv * 3);
    std::vector<int32_t> tris((size_t)nt * 3);
    check(nsk_mesh_download(ctx(), xyz.data(), tris.data()));
    std::vector<uint8_t> rgb;
    if (color && nv > 0) {
        float* d_verts = nullptr; int32_t* d_tris = nullptr;
        check(nsk_mesh_buffers(ctx(), &d_verts, &d_tris));
        DevMem raw((size_t)nv * 4 * sizeof(float));
        const int chunk = (1 << 26) - 1;
        for (long long v0 = 0; v0 < nv; v0 += chunk) {
            const int m = (int)std::min<long long>(chunk, nv - v0);
            check(nsk_eval_points(ctx(), NSK_COLOR, m, d_verts + 3 * v0, (float*)raw.p + 4 * v0));
        }
        check(nsk_sync(ctx()));
        std::vector<float> h((size_t)nv * 4);
        if (hipMemcpy(h.data(), raw.p, h.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("Mesher: D2H failed");
        rgb.resize((size_t)nv * 3);
        for (size_t v = 0; v < (size_t)nv; ++v)
            for (int k = 0; k < 3; ++k) {
                float x = h[4 * v + k];
                x = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;                       // clamp to [0, 1]; NaN -> 0
                rgb[3 * v + k] = (uint8_t)std::lround(x * 255.f);
            }
    }
    Mesher::write_ply(path, xyz.data(), color ? rgb.data() : nullptr, nv, tris.data(), nt);
}

void Mesher::get_mesh(const std::string& path, NICE& decoders, c10::Dict<std::string, torch::Tensor> c, bool color, torch::Tensor valid)
{
    nskh::sync_grids(c);
    decoders.sync_to_device();
    TORCH_CHECK(bound.numel() == 6, "Mesher: bound must be [3,2]");
    check(nsk_set_bound(ctx(), bound.data_ptr<float>()));
    const int n = resolution;
    float origin[3], step[3];
    for (int a = 0; a < 3; ++a) {
        const float lo = bound[a][0].item<float>() - padding, hi = bound[a][1].item<float>() + padding;
        origin[a] = lo;
        step[a] = (hi - lo) / (float)(n - 1);
    }
    const size_t nodes = (size_t)n * n * n;
    DevMem vol(nodes * sizeof(float));
    std::unique_ptr<DevMem> dvalid;
    if (valid.defined()) {
        torch::Tensor h = valid.detach().to(torch::kCPU, torch::kUInt8).contiguous();
        TORCH_CHECK((size_t)h.numel() == nodes, "Mesher: valid must have resolution^3 entries");
        dvalid.reset(new DevMem(nodes));
        if (hipMemcpy(dvalid->p, h.data_ptr<uint8_t>(), nodes, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("Mesher: H2D failed");
    }
    long long n_eval = (long long)nodes;
    if (dvalid) check(nsk_eval_lattice_masked(ctx(), NSK_FINE, origin, step, n, n, n, (const uint8_t*)dvalid->p, 100.f, (float*)vol.p, &n_eval));
    else check(nsk_eval_lattice(ctx(), NSK_FINE, origin, step, n, n, n, (float*)vol.p));
    int nv = 0, nt = 0;
    check(nsk_mesh_extract(ctx(), (const float*)vol.p, dvalid ? (const uint8_t*)dvalid->p : nullptr, n, n, n, origin, step, level_set, &nv, &nt));
    write_context_mesh(path, color, nv, nt);
    last_vertices = nv; last_triangles = nt; last_evaluated = n_eval;
}

void Mesher::get_clean_mesh(const std::string& path, NICE& decoders, c10::Dict<std::string, torch::Tensor> c, const std::vector<torch::Tensor>& depths,
                            const std::vector<torch::Tensor>& c2ws, int H, int W, float fx, float fy, float cx, float cy, bool color)
{
    TORCH_CHECK(depths.size() == c2ws.size(), "Mesher: ", depths.size(), " depth images, ", c2ws.size(), " poses");
    nskh::sync_grids(c);
    decoders.sync_to_device();
    TORCH_CHECK(bound.numel() == 6, "Mesher: bound must be [3,2]");
    check(nsk_set_bound(ctx(), bound.data_ptr<float>()));
    const int n = resolution;
    float origin[3], step[3];
    for (int a = 0; a < 3; ++a) {
        const float lo = bound[a][0].item<float>() - padding, hi = bound[a][1].item<float>() + padding;
        origin[a] = lo;
        step[a] = (hi - lo) / (float)(n - 1);
    }
    const size_t nodes = (size_t)n * n * n, img = (size_t)H * W;
    DevMem vol(nodes * sizeof(float)), seen(nodes);
    // the seen mask, streamed: at most 16 depth images on the device at a time
    const int batch = 16, K = (int)depths.size();
    DevMem dimg((size_t)std::min(std::max(K, 1), batch) * img * sizeof(float));
    std::vector<float> w2c((size_t)batch * 16);
    long long n_seen = 0;
    if (K == 0) check(nsk_lattice_seen(ctx(), origin, step, n, n, n, 0, nullptr, H, W, fx, fy, cx, cy, nullptr, seen_edge, seen_trunc, 0, (uint8_t*)seen.p, &n_seen));
    for (int k0 = 0; k0 < K; k0 += batch) {
        const int kb = std::min(batch, K - k0);
        check(nsk_sync(ctx()));                              // (the previous batch's launch reads the images about to be overwritten)
        for (int k = 0; k < kb; ++k) {
            torch::Tensor d = depths[(size_t)(k0 + k)].detach().to(torch::kCPU, torch::kFloat32).contiguous();
            TORCH_CHECK((size_t)d.numel() == img, "Mesher: depth image ", k0 + k, " is not H x W");
            if (hipMemcpy((float*)dimg.p + (size_t)k * img, d.data_ptr<float>(), img * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("Mesher: H2D failed");
            torch::Tensor m = c2ws[(size_t)(k0 + k)].detach().to(torch::kCPU, torch::kFloat64).contiguous();
            TORCH_CHECK(m.numel() == 16, "Mesher: c2w ", k0 + k, " is not 4 x 4");
            torch::Tensor inv = torch::linalg_inv(m.view({4, 4})).to(torch::kFloat32).contiguous();      // inverted in double, rounded once
            std::memcpy(&w2c[(size_t)k * 16], inv.data_ptr<float>(), 16 * sizeof(float));
        }
        check(nsk_lattice_seen(ctx(), origin, step, n, n, n, kb, (const float*)dimg.p, H, W, fx, fy, cx, cy, w2c.data(), seen_edge, seen_trunc, k0 > 0,
                               (uint8_t*)seen.p, k0 + kb >= K ? &n_seen : nullptr));
    }
    // the decoders run at the seen nodes only: a cell with an unseen corner is not processed, so the extraction never uses the rest
    long long n_eval = 0;
    check(nsk_eval_lattice_masked(ctx(), NSK_FINE, origin, step, n, n, n, (const uint8_t*)seen.p, 100.f, (float*)vol.p, &n_eval));
    int nv = 0, nt = 0, nc = 0, nk = 0;
    check(nsk_mesh_extract(ctx(), (const float*)vol.p, (const uint8_t*)seen.p, n, n, n, origin, step, level_set, &nv, &nt));
    check(nsk_mesh_filter(ctx(), remove_small_geometry_threshold, get_largest_components ? 1 : 0, &nv, &nt, &nc, &nk));
    write_context_mesh(path, color, nv, nt);
    last_vertices = nv; last_triangles = nt; last_components = nc; last_kept = nk; last_seen = n_seen; last_evaluated = n_eval;
}

void Mesher::write_ply(const std::string& path, const float* xyz, const uint8_t* rgb, int nv, const int32_t* tris, int nt)
{
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("Mesher: cannot write " + path);
    std::ostringstream h;
    h << "ply\nformat binary_little_endian 1.0\ncomment nice-slam-cpp_amd Mesher\nelement vertex " << nv
      << "\nproperty float x\nproperty float y\nproperty float z\n";
    if (rgb) h << "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    h << "element face " << nt << "\nproperty list uchar int vertex_indices\nend_header\n";
    const std::string hs = h.str();
    f.write(hs.data(), (std::streamsize)hs.size());
    const size_t vrec = 12 + (rgb ? 3 : 0);
    std::vector<char> buf((size_t)nv * vrec);
    for (size_t v = 0; v < (size_t)nv; ++v) {
        std::memcpy(&buf[v * vrec], xyz + 3 * v, 12);
        if (rgb) std::memcpy(&buf[v * vrec + 12], rgb + 3 * v, 3);
    }
    f.write(buf.data(), (std::streamsize)buf.size());
    buf.resize((size_t)nt * 13);
    for (size_t t = 0; t < (size_t)nt; ++t) {
        buf[t * 13] = 3;
        std::memcpy(&buf[t * 13 + 1], tris + 3 * t, 12);
    }
    f.write(buf.data(), (std::streamsize)buf.size());
    if (!f) throw std::runtime_error("Mesher: write to " + path + " failed");
}

void Mesher::read_ply(const std::string& path, std::vector<float>& xyz, std::vector<uint8_t>& rgb, std::vector<int32_t>& tris)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("Mesher: cannot open " + path);
    std::string line, element;
    long long nv = -1, nt = -1;
    int vprops = 0;
    bool binary = false;
    while (std::getline(f, line)) {
        if (line == "end_header") break;
        std::istringstream ls(line);
        std::string w; ls >> w;
        if (w == "format") { std::string fmt; ls >> fmt; binary = fmt == "binary_little_endian"; }
        else if (w == "element") { ls >> element; if (element == "vertex") ls >> nv; else if (element == "face") ls >> nt; }
        else if (w == "property" && element == "vertex") ++vprops;
    }
    if (!binary || nv < 0 || nt < 0 || (vprops != 3 && vprops != 6)) throw std::runtime_error("Mesher: " + path + " is not a PLY this reader knows");
    const bool color = vprops == 6;
    const size_t vrec = 12 + (color ? 3 : 0);
    std::vector<char> buf((size_t)nv * vrec);
    f.read(buf.data(), (std::streamsize)buf.size());
    xyz.resize((size_t)nv * 3); rgb.resize(color ? (size_t)nv * 3 : 0); tris.resize((size_t)nt * 3);
    for (size_t v = 0; v < (size_t)nv; ++v) {
        std::memcpy(&xyz[3 * v], &buf[v * vrec], 12);
        if (color) std::memcpy(&rgb[3 * v], &buf[v * vrec + 12], 3);
    }
    buf.resize((size_t)nt * 13);
    f.read(buf.data(), (std::streamsize)buf.size());
    if (!f) throw std::runtime_error("Mesher: " + path + " is truncated");
    for (size_t t = 0; t < (size_t)nt; ++t) {
        if (buf[t * 13] != 3) throw std::runtime_error("Mesher: " + path + " has a face that is not a triangle");
        std::memcpy(&tris[3 * t], &buf[t * 13 + 1], 12);
    }
}
