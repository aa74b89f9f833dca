// nsk_mesher.cpp -- Mesher (include/Mesher.h): lattice evaluation and marching cubes stay on the device; the host writes the PLY.
#include "Mesher.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>

#include "nsk_devarr.h"

using nskh::check;
using nskh::ctx;
using nskh::DevArr;

Mesher::Mesher(YAML::Node ns, torch::Tensor bound_3x2, float padding_) : padding(padding_)
{
    resolution = ns["meshing"]["resolution"].IsDefined() ? ns["meshing"]["resolution"].as<int>() : 256;
    level_set = ns["meshing"]["level_set"].IsDefined() ? ns["meshing"]["level_set"].as<float>() : 0.f;
    remove_small_geometry_threshold = ns["meshing"]["remove_small_geometry_threshold"].IsDefined() ? ns["meshing"]["remove_small_geometry_threshold"].as<float>() : 0.2f;
    get_largest_components = ns["meshing"]["get_largest_components"].IsDefined() ? ns["meshing"]["get_largest_components"].as<bool>() : false;
    clean_mesh_bound_scale = ns["meshing"]["clean_mesh_bound_scale"].IsDefined() ? ns["meshing"]["clean_mesh_bound_scale"].as<float>() : 1.02f;
    if (!(clean_mesh_bound_scale > 0.f) || !std::isfinite(clean_mesh_bound_scale)) throw std::runtime_error("Mesher: meshing.clean_mesh_bound_scale must be positive and finite");
    color_method = ns["meshing"]["color_mesh_extraction_method"].IsDefined() ? ns["meshing"]["color_mesh_extraction_method"].as<std::string>() : "direct_point_query";
    if (color_method != "direct_point_query" && color_method != "render_ray_along_normal")
        throw std::runtime_error("Mesher: meshing.color_mesh_extraction_method must be direct_point_query or render_ray_along_normal, not " + color_method);
    if (resolution < 2) throw std::runtime_error("Mesher: meshing.resolution must be at least 2");
    if (!(padding >= 0.f)) throw std::runtime_error("Mesher: padding must be >= 0");
    bound = bound_3x2.defined() ? bound_3x2.detach().to(torch::kCPU, torch::kFloat32).contiguous().clone()
                                : torch::tensor({{-4.5f, 3.82f}, {-1.5f, 2.02f}, {-3.0f, 2.76f}});      // src/Renderer.cpp:15
}

void Mesher::set_bound(torch::Tensor b) { bound = b.detach().to(torch::kCPU, torch::kFloat32).contiguous().clone(); }

namespace {
// the lattice of a Mesher: `resolution` nodes per axis over the bound enlarged by the padding
struct Lattice {
    int n; float origin[3], step[3];
    explicit Lattice(const Mesher& m) : n(m.resolution)
    {
        TORCH_CHECK(m.bound.numel() == 6, "Mesher: bound must be [3,2]");
        for (int a = 0; a < 3; ++a) {
            const float lo = m.bound[a][0].item<float>() - m.padding, hi = m.bound[a][1].item<float>() + m.padding;
            origin[a] = lo;
            step[a] = (hi - lo) / (float)(n - 1);
        }
    }
    size_t nodes() const { return (size_t)n * n * n; }
};

// a mesh on the device: uploaded once per public call
struct DevMesh {
    int nv, nt;
    DevArr<float> v; DevArr<int32_t> t;
    DevMesh(const float* xyz, int nv_, const int32_t* tris, int nt_) : nv(nv_), nt(nt_), v((size_t)nv_ * 3), t((size_t)nt_ * 3)
    {
        v.upload(xyz, (size_t)nv * 3); t.upload(tris, (size_t)nt * 3);
    }
};

// camera-to-world -> world-to-camera: inverted in double, rounded once
void w2c_of(const torch::Tensor& c2w, int k, float* out16)
{
    torch::Tensor m = c2w.detach().to(torch::kCPU, torch::kFloat64).contiguous();
    TORCH_CHECK(m.numel() == 16, "Mesher: c2w ", k, " is not 4 x 4");
    torch::Tensor inv = torch::linalg_inv(m.view({4, 4})).to(torch::kFloat32).contiguous();
    std::memcpy(out16, inv.data_ptr<float>(), 16 * sizeof(float));
}

// K frames as the public calls take them: host tensors (depth [H, W], camera-to-world [4, 4]), or host arrays (depths [K][img] or none,
// world-to-camera [K][16])
struct Frames {
    int K; size_t img;                                   // img = H * W
    const std::vector<torch::Tensor>* depth_t; const std::vector<torch::Tensor>* c2w_t;
    const float* depth_h; const float* w2c_h;
    Frames(const std::vector<torch::Tensor>& depths, const std::vector<torch::Tensor>& c2ws, size_t img_)
        : K((int)depths.size()), img(img_), depth_t(&depths), c2w_t(&c2ws), depth_h(nullptr), w2c_h(nullptr)
    {
        TORCH_CHECK(depths.size() == c2ws.size(), "Mesher: ", depths.size(), " depth images, ", c2ws.size(), " poses");
    }
    Frames(const float* depths, const float* w2c, int K_, size_t img_) : K(K_), img(img_), depth_t(nullptr), c2w_t(nullptr), depth_h(depths), w2c_h(w2c) {}
    // frames [k0, k0 + kb): their images to the front of d (nothing where there are none) -> their [kb][16] world-to-camera rows, made in tmp
    // where the poses came as camera-to-world
    const float* upload(int k0, int kb, DevArr<float>& d, std::vector<float>& tmp) const
    {
        if (!depth_t) {
            if (depth_h) d.upload(depth_h + (size_t)k0 * img, (size_t)kb * img);
            return w2c_h + 16 * (size_t)k0;
        }
        tmp.resize((size_t)kb * 16);
        for (int k = 0; k < kb; ++k) {
            torch::Tensor h = (*depth_t)[(size_t)(k0 + k)].detach().to(torch::kCPU, torch::kFloat32).contiguous();
            TORCH_CHECK((size_t)h.numel() == img, "Mesher: depth image ", k0 + k, " is not H x W");
            d.upload(h.data_ptr<float>(), img, (size_t)k * img);
            w2c_of((*c2w_t)[(size_t)(k0 + k)], k0 + k, &tmp[(size_t)k * 16]);
        }
        return tmp.data();
    }
};

// The frames streamed, at most `batch` depth images on the device at a time: fn(k0, kb, d_depth, w2c) per batch, in order.  d_depth holds
// the batch's images; with images = false it has no element, with frames that carry no images it is fn's own to fill.
template <class Fn>
void stream_frames(const Frames& F, int batch, bool images, Fn fn)
{
    DevArr<float> dimg(images ? (size_t)std::min(std::max(F.K, 1), batch) * F.img : 0);
    std::vector<float> tmp;
    for (int k0 = 0; k0 < F.K; k0 += batch) {
        const int kb = std::min(batch, F.K - k0);
        // (no nsk_sync here: the upload goes through the context's stream, behind the previous batch's launch that reads these images)
        const float* w2c = F.upload(k0, kb, dimg, tmp);
        fn(k0, kb, dimg.p(), w2c);
    }
}
}  // namespace

// the context's mesh (nv vertices, nt triangles) -> host; asked for, the normals and the colours from the device buffers; the PLY
static void write_context_mesh(Mesher& M, const std::string& path, bool color, int nv, int nt)
{
    if (M.color_method != "direct_point_query" && M.color_method != "render_ray_along_normal")
        throw std::runtime_error("Mesher: color_method must be direct_point_query or render_ray_along_normal, not " + M.color_method);
    const bool along = color && M.color_method == "render_ray_along_normal", want_normals = M.write_normals || along;
    if (!(M.simplify_cell >= 0.f) || !std::isfinite(M.simplify_cell)) throw std::runtime_error("Mesher: simplify_cell must be >= 0 and finite");
    // simplify_cell > 0: the context's mesh clustered into buffers of this call (nsk_mesh_simplify); colours and normals are then those of
    // the smaller mesh.  0: the context's mesh as it is
    M.last_simplified_vertices = nv; M.last_simplified_triangles = nt; M.last_collapsed = M.last_duplicates = 0;
    DevArr<float> sv; DevArr<int32_t> st;
    const bool simplified = M.simplify_cell > 0.f;
    if (simplified) {
        float* d_verts = nullptr; int32_t* d_tris = nullptr;
        check(nsk_mesh_buffers(ctx(), &d_verts, &d_tris));
        sv.ensure((size_t)nv * 3); st.ensure((size_t)nt * 3);
        long long info[8];
        check(nsk_mesh_simplify(ctx(), nv > 0 ? d_verts : nullptr, nv, nt > 0 ? d_tris : nullptr, nt, M.simplify_cell, 0, sv.p(), st.p(), nullptr, &nv, &nt, info));
        M.last_simplified_vertices = nv; M.last_simplified_triangles = nt; M.last_collapsed = (int)info[3]; M.last_duplicates = (int)info[4];
    }
    std::vector<float> xyz((size_t)nv * 3);
    std::vector<int32_t> tris((size_t)nt * 3);
    if (simplified) { sv.download(xyz.data(), xyz.size()); st.download(tris.data(), tris.size()); }
    else check(nsk_mesh_download(ctx(), xyz.data(), tris.data()));
    std::vector<uint8_t> rgb;
    std::vector<float> normals;
    M.last_color_fallback = M.last_normals_zero = 0;
    if ((color || want_normals) && nv > 0) {
        float* d_verts = sv.p(); int32_t* d_tris = st.p();
        if (!simplified) check(nsk_mesh_buffers(ctx(), &d_verts, &d_tris));
        const size_t nf = (size_t)nv * 3;
        DevArr<float> dn(want_normals ? nf : 0), raw(color ? nf : 0);
        if (want_normals) {
            int info[4];
            check(nsk_mesh_vertex_normals(ctx(), d_verts, nv, d_tris, nt, dn.p(), info));
            M.last_normals_zero = info[1];
            if (M.write_normals) {
                normals.resize(nf);
                dn.download(normals.data(), nf);
            }
        }
        if (color) {
            check(nsk_mesh_vertex_colors(ctx(), d_verts, nv, along ? dn.p() : nullptr, M.color_ray_length, 0, raw.p(), &M.last_color_fallback));
            std::vector<float> h(nf);
            raw.download(h.data(), nf);
            rgb.resize(nf);
            for (size_t k = 0; k < h.size(); ++k) {
                float x = h[k];
                x = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;                       // clamp to [0, 1]; NaN -> 0
                rgb[k] = (uint8_t)std::lround(x * 255.f);
            }
        }
    }
    static const float none[3] = {0.f, 0.f, 0.f};           // (an empty mesh still declares its normals)
    if (M.write_normals) Mesher::write_ply(path, xyz.data(), nv > 0 ? normals.data() : none, color ? rgb.data() : nullptr, nv, tris.data(), nt);
    else Mesher::write_ply(path, xyz.data(), color ? rgb.data() : nullptr, nv, tris.data(), nt);
}

void Mesher::get_mesh(const std::string& path, NICE& decoders, c10::Dict<std::string, torch::Tensor> c, bool color, torch::Tensor valid)
{
    nskh::sync_grids(c);
    decoders.sync_to_device();
    const Lattice L(*this);
    check(nsk_set_bound(ctx(), bound.data_ptr<float>()));
    const int n = L.n;
    const size_t nodes = L.nodes();
    DevArr<float> vol(nodes);
    DevArr<uint8_t> dvalid;                              // (allocated only with a mask)
    if (valid.defined()) {
        torch::Tensor h = valid.detach().to(torch::kCPU, torch::kUInt8).contiguous();
        TORCH_CHECK((size_t)h.numel() == nodes, "Mesher: valid must have resolution^3 entries");
        dvalid.upload(h.data_ptr<uint8_t>(), nodes);
    }
    long long n_eval = (long long)nodes;
    if (dvalid.p()) check(nsk_eval_lattice_masked(ctx(), NSK_FINE, L.origin, L.step, n, n, n, dvalid.p(), 100.f, vol.p(), &n_eval));
    else check(nsk_eval_lattice(ctx(), NSK_FINE, L.origin, L.step, n, n, n, vol.p()));
    int nv = 0, nt = 0;
    check(nsk_mesh_extract(ctx(), vol.p(), dvalid.p(), n, n, n, L.origin, L.step, level_set, &nv, &nt));
    write_context_mesh(*this, path, color, nv, nt);
    last_vertices = nv; last_triangles = nt; last_evaluated = n_eval;
}

void Mesher::get_clean_mesh(const std::string& path, NICE& decoders, c10::Dict<std::string, torch::Tensor> c, const std::vector<torch::Tensor>& depths,
                            const std::vector<torch::Tensor>& c2ws, int H, int W, float fx, float fy, float cx, float cy, bool color)
{
    const Frames F(depths, c2ws, (size_t)H * W);
    nskh::sync_grids(c);
    decoders.sync_to_device();
    const Lattice L(*this);
    check(nsk_set_bound(ctx(), bound.data_ptr<float>()));
    const int n = L.n, K = F.K;
    DevArr<float> vol(L.nodes());
    DevArr<uint8_t> seen(L.nodes());
    // the seen mask, streamed: at most 16 depth images on the device at a time
    long long n_seen = 0;
    if (K == 0) check(nsk_lattice_seen(ctx(), L.origin, L.step, n, n, n, 0, nullptr, H, W, fx, fy, cx, cy, nullptr, seen_edge, seen_trunc, 0, seen.p(), &n_seen));
    stream_frames(F, 16, true, [&](int k0, int kb, const float* d_depth, const float* w2c) {
        check(nsk_lattice_seen(ctx(), L.origin, L.step, n, n, n, kb, d_depth, H, W, fx, fy, cx, cy, w2c, seen_edge, seen_trunc, k0 > 0, seen.p(),
                               k0 + kb >= K ? &n_seen : nullptr));
    });
    // the decoders run at the seen nodes only: a cell with an unseen corner is not processed, so the extraction never uses the rest
    long long n_eval = 0;
    check(nsk_eval_lattice_masked(ctx(), NSK_FINE, L.origin, L.step, n, n, n, seen.p(), 100.f, vol.p(), &n_eval));
    int nv = 0, nt = 0, nc = 0, nk = 0;
    check(nsk_mesh_extract(ctx(), vol.p(), seen.p(), n, n, n, L.origin, L.step, level_set, &nv, &nt));
    check(nsk_mesh_filter(ctx(), remove_small_geometry_threshold, get_largest_components ? 1 : 0, &nv, &nt, &nc, &nk));
    write_context_mesh(*this, path, color, nv, nt);
    last_vertices = nv; last_triangles = nt; last_components = nc; last_kept = nk; last_seen = n_seen; last_evaluated = n_eval;
}

// ---- depth frames fused into a TSDF, meshed by the extractor ------------------------------------------------------------------------
namespace {
// the fusion of one mesh: the lattice of get_mesh, the volume's buffers, the finish
struct Fusion {
    const Lattice L;
    const int n; float trunc;
    DevArr<float> tsdf, weight;
    Fusion(const Mesher& m, float trunc_steps) : L(m), n(L.n), tsdf(L.nodes()), weight(L.nodes())
    {
        float smax = 0.f;
        for (int a = 0; a < 3; ++a) smax = std::max(smax, L.step[a]);
        trunc = trunc_steps * smax;
    }
    void integrate(const Mesher& m, int K, const float* d_depth, int H, int W, float fx, float fy, float cx, float cy, const float* w2c, bool first,
                   long long* n_observed)
    {
        check(nsk_tsdf_integrate(ctx(), L.origin, L.step, n, n, n, K, d_depth, H, W, fx, fy, cx, cy, w2c, m.seen_edge, trunc, m.fuse_max_weight, first ? 0 : 1,
                                 tsdf.p(), weight.p(), n_observed));
    }
    // volume -> extract -> (asked for) filter; the counts into the Mesher
    void mesh(Mesher& m, float min_weight, int& nv, int& nt)
    {
        DevArr<float> vol(L.nodes());
        DevArr<uint8_t> valid(L.nodes());
        check(nsk_tsdf_volume(ctx(), (long long)L.nodes(), tsdf.p(), weight.p(), min_weight, vol.p(), valid.p(), &m.last_valid));
        check(nsk_mesh_extract(ctx(), vol.p(), valid.p(), n, n, n, L.origin, L.step, 0.f, &nv, &nt));
        m.last_components = m.last_kept = 0;
        if (m.remove_small_geometry_threshold > 0.f || m.get_largest_components)
            check(nsk_mesh_filter(ctx(), m.remove_small_geometry_threshold, m.get_largest_components ? 1 : 0, &nv, &nt, &m.last_components, &m.last_kept));
        m.last_vertices = nv; m.last_triangles = nt;
    }
};
}  // namespace

void Mesher::get_fused_mesh(const std::string& path, const std::vector<torch::Tensor>& depths, const std::vector<torch::Tensor>& c2ws, int H, int W,
                            float fx, float fy, float cx, float cy, float trunc_steps, float min_weight)
{
    const Frames frames(depths, c2ws, (size_t)H * W);
    Fusion F(*this, trunc_steps);
    const int K = frames.K;
    last_observed = 0;
    if (K == 0) F.integrate(*this, 0, nullptr, H, W, fx, fy, cx, cy, nullptr, true, &last_observed);
    stream_frames(frames, 32, true, [&](int k0, int kb, const float* d_depth, const float* w2c) {
        F.integrate(*this, kb, d_depth, H, W, fx, fy, cx, cy, w2c, k0 == 0, k0 + kb >= K ? &last_observed : nullptr);
    });
    int nv = 0, nt = 0;
    F.mesh(*this, min_weight, nv, nt);
    write_context_mesh(*this, path, false, nv, nt);
}

void Mesher::get_hull_mesh(const std::string& path, NICE& decoders, c10::Dict<std::string, torch::Tensor> c, const std::vector<torch::Tensor>& depths,
                           const std::vector<torch::Tensor>& c2ws, int H, int W, float fx, float fy, float cx, float cy, bool color, float trunc_steps,
                           float min_weight)
{
    const Frames frames(depths, c2ws, (size_t)H * W);
    nskh::sync_grids(c);
    decoders.sync_to_device();
    const Lattice L(*this);
    check(nsk_set_bound(ctx(), bound.data_ptr<float>()));
    const int n = L.n, K = frames.K;
    if (!hull_from_context) {
        // the fusion's mesh stays in the context's buffers: the hull reads its vertices there
        Fusion F(*this, trunc_steps);
        last_observed = 0;
        if (K == 0) F.integrate(*this, 0, nullptr, H, W, fx, fy, cx, cy, nullptr, true, &last_observed);
        stream_frames(frames, 32, true, [&](int k0, int kb, const float* d_depth, const float* w2c) {
            F.integrate(*this, kb, d_depth, H, W, fx, fy, cx, cy, w2c, k0 == 0, k0 + kb >= K ? &last_observed : nullptr);
        });
        int fv = 0, ft = 0;
        {
            DevArr<float> fvol(L.nodes());
            DevArr<uint8_t> fvalid(L.nodes());
            check(nsk_tsdf_volume(ctx(), (long long)L.nodes(), F.tsdf.p(), F.weight.p(), min_weight, fvol.p(), fvalid.p(), &last_valid));
            check(nsk_mesh_extract(ctx(), fvol.p(), fvalid.p(), n, n, n, L.origin, L.step, 0.f, &fv, &ft));
        }
        std::vector<float> centres((size_t)K * 3);
        for (int k = 0; k < K; ++k) {
            torch::Tensor m = c2ws[(size_t)k].detach().to(torch::kCPU, torch::kFloat32).contiguous();
            TORCH_CHECK(m.numel() == 16, "Mesher: c2w ", k, " is not 4 x 4");
            for (int a = 0; a < 3; ++a) centres[(size_t)k * 3 + a] = m.data_ptr<float>()[4 * a + 3];
        }
        float* d_verts = nullptr; int32_t* d_tris = nullptr;
        check(nsk_mesh_buffers(ctx(), &d_verts, &d_tris));
        long long info[8];
        check(nsk_points_hull(ctx(), fv > 0 ? d_verts : nullptr, fv, K > 0 ? centres.data() : nullptr, K, info));
        last_hull_vertices.assign((size_t)info[3], 0); last_hull_faces.assign((size_t)info[4] * 3, 0);
        check(nsk_hull_download(ctx(), last_hull_vertices.data(), last_hull_faces.data()));
    }
    DevArr<float> vol(L.nodes());
    DevArr<uint8_t> inside(L.nodes());
    check(nsk_lattice_in_hull(ctx(), L.origin, L.step, n, n, n, (double)clean_mesh_bound_scale, 0, inside.p(), &last_inside));
    long long n_eval = 0;
    check(nsk_eval_lattice_masked(ctx(), NSK_FINE, L.origin, L.step, n, n, n, inside.p(), 100.f, vol.p(), &n_eval));
    int nv = 0, nt = 0;
    check(nsk_mesh_extract(ctx(), vol.p(), inside.p(), n, n, n, L.origin, L.step, level_set, &nv, &nt));
    write_context_mesh(*this, path, color, nv, nt);
    last_vertices = nv; last_triangles = nt; last_evaluated = n_eval;
}

void Mesher::get_rendered_mesh(const std::string& path, NICE& decoders, c10::Dict<std::string, torch::Tensor> c, const std::vector<torch::Tensor>& depths,
                               const std::vector<torch::Tensor>& c2ws, int H, int W, float fx, float fy, float cx, float cy, float trunc_steps,
                               float min_weight, bool color, const std::string& stage, int chunk_rays)
{
    TORCH_CHECK(depths.empty() || depths.size() == c2ws.size(), "Mesher: ", depths.size(), " depth images, ", c2ws.size(), " poses");
    nskh::sync_grids(c);
    decoders.sync_to_device();
    TORCH_CHECK(bound.numel() == 6, "Mesher: bound must be [3,2]");
    check(nsk_set_bound(ctx(), bound.data_ptr<float>()));
    Fusion F(*this, trunc_steps);
    const size_t img = (size_t)H * W;
    const int K = (int)c2ws.size();
    DevArr<float> guide(img), pose(12), rgb(img * 3), depth(img), var(img);
    last_observed = 0;
    F.integrate(*this, 0, nullptr, H, W, fx, fy, cx, cy, nullptr, true, K == 0 ? &last_observed : nullptr);        // (cleared)
    float w2c[16];
    for (int k = 0; k < K; ++k) {
        // (no nsk_sync here: the uploads go through the context's stream, behind the previous frame's launches that read these buffers)
        torch::Tensor m = c2ws[(size_t)k].detach().to(torch::kCPU, torch::kFloat32).contiguous();
        TORCH_CHECK(m.numel() == 16, "Mesher: c2w ", k, " is not 4 x 4");
        pose.upload(m.data_ptr<float>(), 12);
        if (!depths.empty()) {
            torch::Tensor d = depths[(size_t)k].detach().to(torch::kCPU, torch::kFloat32).contiguous();
            TORCH_CHECK((size_t)d.numel() == img, "Mesher: depth image ", k, " is not H x W");
            guide.upload(d.data_ptr<float>(), img);
        }
        check(nsk_render_image(ctx(), nskh::stage_id(stage), 0, H, 0, W, 1, H, W, fx, fy, cx, cy, pose.p(), 0, 0, depths.empty() ? nullptr : guide.p(), -1.f,
                               chunk_rays, rgb.p(), depth.p(), var.p()));
        w2c_of(c2ws[(size_t)k], k, w2c);
        F.integrate(*this, 1, depth.p(), H, W, fx, fy, cx, cy, w2c, false, k + 1 == K ? &last_observed : nullptr);
    }
    int nv = 0, nt = 0;
    F.mesh(*this, min_weight, nv, nt);
    write_context_mesh(*this, path, color, nv, nt);
}

void Mesher::write_ply(const std::string& path, const float* xyz, const uint8_t* rgb, int nv, const int32_t* tris, int nt)
{
    write_ply(path, xyz, nullptr, rgb, nv, tris, nt);
}

void Mesher::write_ply(const std::string& path, const float* xyz, const float* normals, const uint8_t* rgb, int nv, const int32_t* tris, int nt)
{
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("Mesher: cannot write " + path);
    std::ostringstream h;
    h << "ply\nformat binary_little_endian 1.0\ncomment nice-slam-cpp_amd Mesher\nelement vertex " << nv
      << "\nproperty float x\nproperty float y\nproperty float z\n";
    if (normals) h << "property float nx\nproperty float ny\nproperty float nz\n";
    if (rgb) h << "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    h << "element face " << nt << "\nproperty list uchar int vertex_indices\nend_header\n";
    const std::string hs = h.str();
    f.write(hs.data(), (std::streamsize)hs.size());
    const size_t noff = 12, coff = noff + (normals ? 12 : 0), vrec = coff + (rgb ? 3 : 0);
    std::vector<char> buf((size_t)nv * vrec);
    for (size_t v = 0; v < (size_t)nv; ++v) {
        std::memcpy(&buf[v * vrec], xyz + 3 * v, 12);
        if (normals) std::memcpy(&buf[v * vrec + noff], normals + 3 * v, 12);
        if (rgb) std::memcpy(&buf[v * vrec + coff], rgb + 3 * v, 3);
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

// the files write_ply writes: x y z, then nx ny nz and red green blue when `with_normals` / 3 further properties say so
static void read_own_ply(const std::string& path, bool with_normals, std::vector<float>& xyz, std::vector<float>* normals, std::vector<uint8_t>& rgb,
                         std::vector<int32_t>& tris)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("Mesher: cannot open " + path);
    std::string line, element;
    long long nv = -1, nt = -1;
    std::vector<std::string> vprops;
    bool binary = false;
    while (std::getline(f, line)) {
        if (line == "end_header") break;
        std::istringstream ls(line);
        std::string w; ls >> w;
        if (w == "format") { std::string fmt; ls >> fmt; binary = fmt == "binary_little_endian"; }
        else if (w == "element") { ls >> element; if (element == "vertex") ls >> nv; else if (element == "face") ls >> nt; }
        else if (w == "property" && element == "vertex") { std::string t, name; ls >> t >> name; vprops.push_back(t + " " + name); }
    }
    const std::vector<std::string> P = {"float x", "float y", "float z"}, N = {"float nx", "float ny", "float nz"},
                                   C = {"uchar red", "uchar green", "uchar blue"};
    auto at = [&](size_t k, const std::vector<std::string>& want) {
        return vprops.size() >= k + 3 && std::equal(want.begin(), want.end(), vprops.begin() + (std::ptrdiff_t)k);
    };
    bool known = binary && nv >= 0 && nt >= 0 && (with_normals ? at(0, P) : vprops.size() >= 3);
    const bool has_n = with_normals && at(3, N);
    const size_t coff = 12 + (has_n ? 12 : 0), nprop = 3 + (has_n ? 3 : 0);
    const bool color = with_normals ? at(nprop, C) : vprops.size() == 6;
    known = known && vprops.size() == nprop + (color ? 3 : 0);
    if (!known) throw std::runtime_error("Mesher: " + path + " is not a PLY this reader knows");
    const size_t vrec = coff + (color ? 3 : 0);
    std::vector<char> buf((size_t)nv * vrec);
    f.read(buf.data(), (std::streamsize)buf.size());
    xyz.resize((size_t)nv * 3); rgb.resize(color ? (size_t)nv * 3 : 0); tris.resize((size_t)nt * 3);
    if (normals) normals->resize(has_n ? (size_t)nv * 3 : 0);
    for (size_t v = 0; v < (size_t)nv; ++v) {
        std::memcpy(&xyz[3 * v], &buf[v * vrec], 12);
        if (has_n) std::memcpy(&(*normals)[3 * v], &buf[v * vrec + 12], 12);
        if (color) std::memcpy(&rgb[3 * v], &buf[v * vrec + coff], 3);
    }
    buf.resize((size_t)nt * 13);
    f.read(buf.data(), (std::streamsize)buf.size());
    if (!f) throw std::runtime_error("Mesher: " + path + " is truncated");
    for (size_t t = 0; t < (size_t)nt; ++t) {
        if (buf[t * 13] != 3) throw std::runtime_error("Mesher: " + path + " has a face that is not a triangle");
        std::memcpy(&tris[3 * t], &buf[t * 13 + 1], 12);
    }
}

void Mesher::read_ply(const std::string& path, std::vector<float>& xyz, std::vector<uint8_t>& rgb, std::vector<int32_t>& tris)
{
    read_own_ply(path, false, xyz, nullptr, rgb, tris);
}

void Mesher::read_ply(const std::string& path, std::vector<float>& xyz, std::vector<float>& normals, std::vector<uint8_t>& rgb, std::vector<int32_t>& tris)
{
    read_own_ply(path, true, xyz, &normals, rgb, tris);
}

// ---- any PLY mesh ------------------------------------------------------------------------------------------------------------------
namespace {
struct PlyProp { std::string name; int type = -1, count_type = -1; bool list = false; };       // types: index into PLY_TYPES
struct PlyElem { std::string name; long long count = 0; std::vector<PlyProp> props; };
const struct { const char* a; const char* b; int size; } PLY_TYPES[] = {
    {"char", "int8", 1}, {"uchar", "uint8", 1}, {"short", "int16", 2}, {"ushort", "uint16", 2},
    {"int", "int32", 4}, {"uint", "uint32", 4}, {"float", "float32", 4}, {"double", "float64", 8}};
int ply_type(const std::string& w)
{
    for (int k = 0; k < 8; ++k) if (w == PLY_TYPES[k].a || w == PLY_TYPES[k].b) return k;
    return -1;
}
// one scalar of type t from the body
struct PlyBody {
    const std::string& path; const char* p; const char* end; bool ascii;
    [[noreturn]] void truncated() const { throw std::runtime_error("Mesher: " + path + " is truncated"); }
    double next(int t)
    {
        if (ascii) {
            while (p < end && (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t')) ++p;
            if (p >= end) truncated();
            const char* q = p;
            while (q < end && !(*q == ' ' || *q == '\n' || *q == '\r' || *q == '\t')) ++q;
            const std::string tok(p, q);
            p = q;
            char* e = nullptr;
            const double v = std::strtod(tok.c_str(), &e);
            if (e == tok.c_str() || *e) throw std::runtime_error("Mesher: " + path + " has '" + tok + "' where a number belongs");
            return v;
        }
        const int n = PLY_TYPES[t].size;
        if (end - p < n) truncated();
        double v = 0;
        switch (t) {
            case 0: { int8_t x; std::memcpy(&x, p, 1); v = x; break; }
            case 1: { uint8_t x; std::memcpy(&x, p, 1); v = x; break; }
            case 2: { int16_t x; std::memcpy(&x, p, 2); v = x; break; }
            case 3: { uint16_t x; std::memcpy(&x, p, 2); v = x; break; }
            case 4: { int32_t x; std::memcpy(&x, p, 4); v = x; break; }
            case 5: { uint32_t x; std::memcpy(&x, p, 4); v = x; break; }
            case 6: { float x; std::memcpy(&x, p, 4); v = x; break; }
            default: { double x; std::memcpy(&x, p, 8); v = x; break; }
        }
        p += n;
        return v;
    }
};
}  // namespace

void Mesher::read_ply_mesh(const std::string& path, std::vector<float>& xyz, std::vector<int32_t>& tris)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("Mesher: cannot open " + path);
    const std::string all((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    auto bad = [&](const std::string& why) { return std::runtime_error("Mesher: " + path + ": " + why); };
    // the header, line by line
    size_t pos = 0;
    bool first = true, ended = false, ascii = false, have_format = false;
    std::vector<PlyElem> elems;
    while (pos < all.size()) {
        size_t nl = all.find('\n', pos);
        if (nl == std::string::npos) break;
        std::string line = all.substr(pos, nl - pos);
        pos = nl + 1;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (first) { if (line != "ply") throw bad("not a PLY file"); first = false; continue; }
        if (line == "end_header") { ended = true; break; }
        std::istringstream ls(line);
        std::string w; ls >> w;
        if (w == "format") {
            std::string fmt; ls >> fmt;
            if (fmt == "ascii") ascii = true;
            else if (fmt == "binary_little_endian") ascii = false;
            else if (fmt == "binary_big_endian") throw bad("big-endian PLY files are not read");
            else throw bad("unknown format '" + fmt + "'");
            have_format = true;
        } else if (w == "element") {
            PlyElem e; ls >> e.name >> e.count;
            if (!ls || e.count < 0) throw bad("malformed element line '" + line + "'");
            elems.push_back(e);
        } else if (w == "property") {
            if (elems.empty()) throw bad("a property before any element");
            PlyProp p; std::string t; ls >> t;
            if (t == "list") { std::string ct, it; ls >> ct >> it >> p.name; p.list = true; p.count_type = ply_type(ct); p.type = ply_type(it); }
            else { ls >> p.name; p.type = ply_type(t); }
            if (!ls || p.type < 0 || (p.list && (p.count_type < 0 || p.count_type > 5))) throw bad("malformed property line '" + line + "'");
            elems.back().props.push_back(p);
        }       // comment, obj_info: skipped
    }
    if (first || !ended) throw bad(first ? "not a PLY file" : "the header does not end (truncated)");
    if (!have_format) throw bad("no format line");
    const PlyElem* ve = nullptr; const PlyElem* fe = nullptr;
    for (const PlyElem& e : elems) { if (e.name == "vertex") ve = &e; else if (e.name == "face") fe = &e; }
    if (!ve) throw bad("no vertex element");
    int ix[3] = {-1, -1, -1};
    for (size_t k = 0; k < ve->props.size(); ++k)
        for (int a = 0; a < 3; ++a)
            if (!ve->props[k].list && ve->props[k].name == std::string(1, (char)('x' + a)) && ix[a] < 0) ix[a] = (int)k;
    if (ix[0] < 0 || ix[1] < 0 || ix[2] < 0) throw bad("the vertex element has no scalar x, y, z");
    if (ve->count > 0x7fffffffLL) throw bad("more than 2^31 - 1 vertices");
    int flist = -1;
    if (fe) for (size_t k = 0; k < fe->props.size() && flist < 0; ++k) if (fe->props[k].list) flist = (int)k;
    xyz.assign((size_t)ve->count * 3, 0.f);
    tris.clear();
    PlyBody B{path, all.data() + pos, all.data() + all.size(), ascii};
    bool seen_vertices = false;
    std::vector<long long> poly;
    for (const PlyElem& e : elems) {
        const bool is_v = &e == ve, is_f = &e == fe && flist >= 0;
        if (is_f && !seen_vertices) throw bad("the face element comes before the vertex element");
        for (long long r = 0; r < e.count; ++r)
            for (size_t k = 0; k < e.props.size(); ++k) {
                const PlyProp& p = e.props[k];
                if (!p.list) {
                    const double v = B.next(p.type);
                    if (is_v) for (int a = 0; a < 3; ++a) if (ix[a] == (int)k) xyz[3 * (size_t)r + a] = (float)v;
                    continue;
                }
                const double cnt = B.next(p.count_type);
                if (!(cnt >= 0) || cnt != std::floor(cnt)) throw bad("a list with a count that is no whole number");
                const long long m = (long long)cnt;
                const bool take = is_f && (int)k == flist;
                poly.clear();
                for (long long q = 0; q < m; ++q) {
                    const double v = B.next(p.type);
                    if (!take) continue;
                    if (!(v >= 0 && v < (double)ve->count) || v != std::floor(v))
                        throw bad("face " + std::to_string(r) + " has an index outside the " + std::to_string(ve->count) + " vertices");
                    poly.push_back((long long)v);
                }
                for (size_t q = 1; take && q + 1 < poly.size(); ++q) {
                    tris.push_back((int32_t)poly[0]); tris.push_back((int32_t)poly[q]); tris.push_back((int32_t)poly[q + 1]);
                }
            }
        if (is_v) seen_vertices = true;
    }
}

// ---- alignment -------------------------------------------------------------------------------------------------------------------------
// align_recon on vertices that are on the device already
static ReconAlign align_device(const float* d_rec, int rec_nv, const float* d_gt, int gt_nv, float threshold = 0.1f, int max_iter = 30)
{
    if (rec_nv < 1 || gt_nv < 1) throw std::runtime_error("Mesher::align_recon: a mesh without a vertex");
    ReconAlign A;
    double info[8];
    check(nsk_cloud_icp(ctx(), d_rec, rec_nv, d_gt, gt_nv, threshold, max_iter, 1e-6, 1e-6, nullptr, A.transform, info));
    A.iterations = (int)info[0]; A.fitness = info[1]; A.rmse = info[2]; A.correspondences = (int)info[3];
    A.converged = info[4] != 0.0; A.degenerate = info[7] != 0.0;
    return A;
}
ReconAlign Mesher::align_recon(const float* rec_xyz, int rec_nv, const float* gt_xyz, int gt_nv, float threshold, int max_iter)
{
    if (rec_nv < 1 || gt_nv < 1) throw std::runtime_error("Mesher::align_recon: a mesh without a vertex");
    DevArr<float> rv((size_t)rec_nv * 3), gv((size_t)gt_nv * 3);
    rv.upload(rec_xyz, (size_t)rec_nv * 3); gv.upload(gt_xyz, (size_t)gt_nv * 3);
    return align_device(rv.p(), rec_nv, gv.p(), gt_nv, threshold, max_iter);
}
// the reconstruction registered to the ground truth where it lies, on the device; the fields both results share
template <class R> static void align_on_device(R& M, DevMesh& rec, const DevMesh& gt)
{
    const ReconAlign A = align_device(rec.v.p(), rec.nv, gt.v.p(), gt.nv);
    for (int k = 0; k < 16; ++k) M.transform[k] = A.transform[k];
    M.icp_fitness = A.fitness; M.icp_rmse = A.rmse; M.icp_iterations = A.iterations;
    check(nsk_cloud_transform(ctx(), M.transform, rec.v.p(), rec.nv, rec.v.p()));
}

// ---- reconstruction metrics ----------------------------------------------------------------------------------------------------------
ReconMetrics Mesher::eval_recon(const float* rec_xyz, int rec_nv, const int32_t* rec_tris, int rec_nt, const float* gt_xyz, int gt_nv,
                                const int32_t* gt_tris, int gt_nt, int n, float threshold, unsigned long long seed, bool align, bool surface)
{
    if (n < 1) throw std::runtime_error("Mesher::eval_recon: n_points must be at least 1");
    if (rec_nt < 1 || gt_nt < 1) throw std::runtime_error("Mesher::eval_recon: a mesh without a triangle");
    ReconMetrics M;
    DevArr<float> rec_pts((size_t)n * 3), gt_pts((size_t)n * 3), dist((size_t)n);
    const double nan = std::nan("");
    double a[4], c[4];
    if (surface) {      // both meshes stay on the device: every sample is measured against the other mesh's triangles
        DevMesh rec(rec_xyz, rec_nv, rec_tris, rec_nt), gt(gt_xyz, gt_nv, gt_tris, gt_nt);
        DevArr<int32_t> own((size_t)n), gt_own((size_t)n), hit((size_t)n);
        if (align) align_on_device(M, rec, gt);
        const float *RV = rec.v.p(), *GV = gt.v.p();
        const int32_t *RT = rec.t.p(), *GT = gt.t.p();
        check(nsk_mesh_sample(ctx(), RV, rec_nv, RT, rec_nt, seed, n, rec_pts.p(), own.p(), &M.rec_area, &M.rec_degenerate));
        check(nsk_mesh_sample(ctx(), GV, gt_nv, GT, gt_nt, seed + 1, n, gt_pts.p(), gt_own.p(), &M.gt_area, &M.gt_degenerate));
        double na[3], nc[3];
        check(nsk_mesh_nearest(ctx(), rec_pts.p(), n, GV, gt_nv, GT, gt_nt, dist.p(), hit.p(), nullptr, &M.gt_skipped));
        check(nsk_cloud_stats(ctx(), dist.p(), n, threshold, a));
        check(nsk_normal_stats(ctx(), n, RV, rec_nv, RT, rec_nt, own.p(), GV, gt_nv, GT, gt_nt, hit.p(), na));
        check(nsk_mesh_nearest(ctx(), gt_pts.p(), n, RV, rec_nv, RT, rec_nt, dist.p(), hit.p(), nullptr, &M.rec_skipped));
        check(nsk_cloud_stats(ctx(), dist.p(), n, threshold, c));
        check(nsk_normal_stats(ctx(), n, GV, gt_nv, GT, gt_nt, gt_own.p(), RV, rec_nv, RT, rec_nt, hit.p(), nc));
        check(nsk_sync(ctx()));
        M.surface = true;
        M.precision_pct = a[1] > 0 ? 100.0 * a[2] / a[1] : nan;
        M.recall_pct = c[1] > 0 ? 100.0 * c[2] / c[1] : nan;
        const double pr = M.precision_pct + M.recall_pct;
        M.fscore_pct = pr > 0 ? 2.0 * M.precision_pct * M.recall_pct / pr : (pr == 0 ? 0.0 : nan);
        M.normal_accuracy = na[1] > 0 ? na[0] / na[1] : nan;
        M.normal_completion = nc[1] > 0 ? nc[0] / nc[1] : nan;
        M.normal_consistency = 0.5 * (M.normal_accuracy + M.normal_completion);
        M.normal_skipped = (int)(na[2] + nc[2]);
    } else {
        {   // the meshes leave the device again as soon as their samples are drawn
            DevMesh rec(rec_xyz, rec_nv, rec_tris, rec_nt), gt(gt_xyz, gt_nv, gt_tris, gt_nt);
            if (align) align_on_device(M, rec, gt);
            check(nsk_mesh_sample(ctx(), rec.v.p(), rec_nv, rec.t.p(), rec_nt, seed, n, rec_pts.p(), nullptr, &M.rec_area, &M.rec_degenerate));
            check(nsk_mesh_sample(ctx(), gt.v.p(), gt_nv, gt.t.p(), gt_nt, seed + 1, n, gt_pts.p(), nullptr, &M.gt_area, &M.gt_degenerate));
            check(nsk_sync(ctx()));
        }
        check(nsk_cloud_nearest(ctx(), rec_pts.p(), n, gt_pts.p(), n, dist.p(), nullptr, &M.gt_skipped));
        check(nsk_cloud_stats(ctx(), dist.p(), n, threshold, a));
        check(nsk_cloud_nearest(ctx(), gt_pts.p(), n, rec_pts.p(), n, dist.p(), nullptr, &M.rec_skipped));
        check(nsk_cloud_stats(ctx(), dist.p(), n, threshold, c));
    }
    M.accuracy_cm = a[1] > 0 ? 100.0 * a[0] / a[1] : nan;
    M.completion_cm = c[1] > 0 ? 100.0 * c[0] / c[1] : nan;
    M.completion_ratio_pct = c[1] > 0 ? 100.0 * c[2] / c[1] : nan;
    M.accuracy_max_cm = 100.0 * a[3]; M.completion_max_cm = 100.0 * c[3];
    return M;
}

ReconMetrics Mesher::eval_recon(const std::string& rec_ply, const std::string& gt_ply, int n, float threshold, unsigned long long seed, bool align,
                                bool surface)
{
    std::vector<float> rv, gv;
    std::vector<int32_t> rt, gt;
    read_ply_mesh(rec_ply, rv, rt);
    read_ply_mesh(gt_ply, gv, gt);
    if (rt.empty()) throw std::runtime_error("Mesher::eval_recon: " + rec_ply + " has no triangle");
    if (gt.empty()) throw std::runtime_error("Mesher::eval_recon: " + gt_ply + " has no triangle");
    return eval_recon(rv.data(), (int)(rv.size() / 3), rt.data(), (int)(rt.size() / 3), gv.data(), (int)(gv.size() / 3), gt.data(), (int)(gt.size() / 3),
                      n, threshold, seed, align, surface);
}

// ---- reconstruction depth L1 -----------------------------------------------------------------------------------------------------------
ReconDepth Mesher::eval_recon_depth(const float* rec_xyz, int rec_nv, const int32_t* rec_tris, int rec_nt, const float* gt_xyz, int gt_nv,
                                    const int32_t* gt_tris, int gt_nt, int n_views, int H, int W, float focal, unsigned long long seed,
                                    double shrink, double min_cover, bool align, const float* unseen_xyz, int n_unseen)
{
    if (n_views < 1) throw std::runtime_error("Mesher::eval_recon_depth: n_views must be at least 1");
    if (H < 1 || W < 1 || (long long)H * W > (1LL << 24)) throw std::runtime_error("Mesher::eval_recon_depth: the image must have 1 .. 2^24 pixels");
    if (gt_nv < 1) throw std::runtime_error("Mesher::eval_recon_depth: the ground truth has no vertex");
    const size_t n_pix = (size_t)H * W;
    DevMesh rec(rec_xyz, rec_nv, rec_tris, rec_nt), gt(gt_xyz, gt_nv, gt_tris, gt_nt);
    ReconDepth M;
    if (align) align_on_device(M, rec, gt);
    const float cx = (float)(W / 2.0 - 0.5), cy = (float)(H / 2.0 - 0.5);
    float box[6];
    if (unseen_xyz && n_unseen > 0) {
        // upstream's redraw: the first n_views candidates of the stream without an unseen point in their image, counted in rounds
        const int round = 32, cap_factor = 16;
        const long long cap = (long long)cap_factor * n_views;
        DevArr<float> unseen((size_t)n_unseen * 3);
        unseen.upload(unseen_xyz, (size_t)n_unseen * 3);
        check(nsk_depth_views(ctx(), gt.v.p(), gt_nv, box, seed, shrink, 0, nullptr));        // (the box)
        std::vector<float> w((size_t)round * 16);
        std::vector<long long> cnt((size_t)round);
        long long first = 0;
        while ((int)M.view_index.size() < n_views && first < cap) {
            const int m = (int)std::min<long long>(round, cap - first);
            check(nsk_depth_views_range(box, seed, shrink, first, m, w.data()));
            check(nsk_points_view_counts(ctx(), unseen.p(), n_unseen, m, w.data(), H, W, focal, focal, cx, cy, 0, cnt.data()));
            for (int k = 0; k < m && (int)M.view_index.size() < n_views; ++k) {
                if (cnt[(size_t)k] != 0) continue;
                M.view_index.push_back(first + k);
                M.w2c.insert(M.w2c.end(), w.begin() + 16 * (size_t)k, w.begin() + 16 * (size_t)(k + 1));
            }
            first += m;
        }
        M.candidates_tried = (int)M.view_index.size() == n_views ? (int)(M.view_index.back() + 1) : (int)cap;
        n_views = (int)M.view_index.size();
    } else {
        M.w2c.assign((size_t)n_views * 16, 0.f);
        check(nsk_depth_views(ctx(), gt.v.p(), gt_nv, box, seed, shrink, n_views, M.w2c.data()));
    }
    M.n_views = n_views;
    M.stats.assign((size_t)n_views * 4, 0.0);
    int batch = (int)std::max<size_t>(1, ((size_t)1 << 27) / n_pix);          // both stacks together stay below about 1 GB
    if (batch > 32) batch -= batch % 32;
    batch = std::max(1, std::min(batch, n_views));
    DevArr<float> dg((size_t)batch * n_pix), dr((size_t)batch * n_pix);
    for (int k0 = 0; k0 < n_views; k0 += batch) {
        const int V = std::min(batch, n_views - k0);
        const float* w = M.w2c.data() + 16 * (size_t)k0;
        check(nsk_mesh_depth(ctx(), gt.v.p(), gt_nv, gt.t.p(), gt_nt, V, w, H, W, focal, focal, cx, cy, dg.p(), k0 == 0 ? &M.gt_skipped : nullptr));
        check(nsk_mesh_depth(ctx(), rec.v.p(), rec_nv, rec.t.p(), rec_nt, V, w, H, W, focal, focal, cx, cy, dr.p(), k0 == 0 ? &M.rec_skipped : nullptr));
        check(nsk_depth_pair_stats(ctx(), dg.p(), dr.p(), V, (int)n_pix, M.stats.data() + 4 * (size_t)k0));
    }
    M.view_l1.resize((size_t)n_views); M.view_cover.resize((size_t)n_views);
    double l1 = 0.0, both = 0.0, both_sum = 0.0;
    for (int k = 0; k < n_views; ++k) {
        const double* s = &M.stats[4 * (size_t)k];
        M.view_l1[k] = s[0] / (double)n_pix; M.view_cover[k] = s[3] / (double)n_pix;
        if (!(M.view_cover[k] >= min_cover)) continue;
        ++M.n_used; l1 += M.view_l1[k]; both += s[1]; both_sum += s[2];
    }
    const double nan = std::nan("");
    M.depth_l1_cm = M.n_used ? 100.0 * l1 / M.n_used : nan;
    M.restricted_l1_cm = both > 0 ? 100.0 * both_sum / both : nan;
    return M;
}

ReconDepth Mesher::eval_recon_depth(const std::string& rec_ply, const std::string& gt_ply, int n_views, int H, int W, float focal,
                                    unsigned long long seed, double shrink, double min_cover, bool align)
{
    std::vector<float> rv, gv;
    std::vector<int32_t> rt, gt;
    read_ply_mesh(rec_ply, rv, rt);
    read_ply_mesh(gt_ply, gv, gt);
    return eval_recon_depth(rv.data(), (int)(rv.size() / 3), rt.data(), (int)(rt.size() / 3), gv.data(), (int)(gv.size() / 3), gt.data(),
                            (int)(gt.size() / 3), n_views, H, W, focal, seed, shrink, min_cover, align);
}

// ---- culling to what a trajectory saw -----------------------------------------------------------------------------------------------------
CulledMesh Mesher::cull_mesh(const float* xyz, int nv, const int32_t* tris, int nt, const float* w2c, int K, int H, int W, float fx, float fy,
                             float cx, float cy, const float* depths, const std::string& occlusion, int edge, float eps, int frames_per_batch)
{
    const int mode = occlusion == "none" ? 0 : occlusion == "depth" ? 1 : occlusion == "self" ? 2 : -1;
    if (mode < 0) throw std::runtime_error("Mesher::cull_mesh: occlusion must be none, depth or self, not " + occlusion);
    if (nv < 0 || nt < 0 || K < 0) throw std::runtime_error("Mesher::cull_mesh: negative count");
    if (H < 1 || W < 1 || (long long)H * W > (1LL << 24)) throw std::runtime_error("Mesher::cull_mesh: the image must have 1 .. 2^24 pixels");
    if (mode == 1 && K > 0 && !depths) throw std::runtime_error("Mesher::cull_mesh: occlusion depth needs the depth images");
    const DevMesh in(xyz, nv, tris, nt);
    DevArr<uint8_t> seen((size_t)nv);
    DevArr<float> ov((size_t)nv * 3);
    DevArr<int32_t> ot((size_t)nt * 3), src((size_t)nv);
    CulledMesh R;
    check(nsk_points_seen(ctx(), in.v.p(), nv, 0, nullptr, H, W, fx, fy, cx, cy, nullptr, edge, eps, 0, 0, seen.p(), nullptr));     // (cleared)
    // depth: the sensor's images are streamed;  self: every batch's images are rendered from the mesh into the streamer's buffer;  none: no images
    const Frames frames(mode == 1 ? depths : nullptr, w2c, K, (size_t)H * W);
    stream_frames(frames, std::max(1, frames_per_batch), mode != 0, [&](int k0, int kb, float* d_depth, const float* w) {
        if (mode == 2) check(nsk_mesh_depth(ctx(), in.v.p(), nv, in.t.p(), nt, kb, w, H, W, fx, fy, cx, cy, d_depth, nullptr));
        check(nsk_points_seen(ctx(), in.v.p(), nv, kb, mode == 0 ? nullptr : d_depth, H, W, fx, fy, cx, cy, w, edge, eps, mode == 2 ? 1 : 0, 1, seen.p(),
                              k0 + kb >= K ? &R.n_seen : nullptr));
    });
    int onv = 0, ont = 0;
    check(nsk_mesh_select(ctx(), in.v.p(), nv, in.t.p(), nt, seen.p(), 0, ov.p(), ot.p(), src.p(), &onv, &ont, &R.skipped));
    R.xyz.resize((size_t)onv * 3); R.triangles.resize((size_t)ont * 3); R.vertex_src.resize((size_t)onv); R.seen.resize((size_t)nv);
    ov.download(R.xyz.data(), R.xyz.size()); ot.download(R.triangles.data(), R.triangles.size());
    src.download(R.vertex_src.data(), R.vertex_src.size()); seen.download(R.seen.data(), R.seen.size());
    return R;
}

CulledMesh Mesher::cull_mesh(const std::string& in_ply, const std::string& out_ply, const float* w2c, int K, int H, int W, float fx, float fy,
                             float cx, float cy, const float* depths, const std::string& occlusion, int edge, float eps, int frames_per_batch)
{
    std::vector<float> xyz;
    std::vector<int32_t> tris;
    read_ply_mesh(in_ply, xyz, tris);
    CulledMesh R = cull_mesh(xyz.data(), (int)(xyz.size() / 3), tris.data(), (int)(tris.size() / 3), w2c, K, H, W, fx, fy, cx, cy, depths, occlusion,
                             edge, eps, frames_per_batch);
    write_ply(out_ply, R.xyz.data(), nullptr, (int)(R.xyz.size() / 3), R.triangles.data(), (int)(R.triangles.size() / 3));
    return R;
}

// ---- a mesh made smaller: vertex clustering -------------------------------------------------------------------------------------------------
SimplifiedMesh Mesher::simplify_mesh(const float* xyz, int nv, const int32_t* tris, int nt, float cell, bool keep_duplicates)
{
    if (nv < 0 || nt < 0) throw std::runtime_error("Mesher::simplify_mesh: negative count");
    const DevMesh in(xyz, nv, tris, nt);
    DevArr<float> ov((size_t)nv * 3);
    DevArr<int32_t> ot((size_t)nt * 3), vmap((size_t)nv);
    SimplifiedMesh R;
    int onv = 0, ont = 0;
    check(nsk_mesh_simplify(ctx(), nv > 0 ? in.v.p() : nullptr, nv, nt > 0 ? in.t.p() : nullptr, nt, cell, keep_duplicates ? 1 : 0, ov.p(), ot.p(), vmap.p(),
                            &onv, &ont, R.info));
    R.xyz.resize((size_t)onv * 3); R.triangles.resize((size_t)ont * 3); R.vertex_map.resize((size_t)nv);
    ov.download(R.xyz.data(), R.xyz.size()); ot.download(R.triangles.data(), R.triangles.size()); vmap.download(R.vertex_map.data(), R.vertex_map.size());
    return R;
}

SimplifiedMesh Mesher::simplify_mesh(const std::string& in_ply, const std::string& out_ply, float cell, bool keep_duplicates)
{
    std::vector<float> xyz;
    std::vector<int32_t> tris;
    read_ply_mesh(in_ply, xyz, tris);
    SimplifiedMesh R = simplify_mesh(xyz.data(), (int)(xyz.size() / 3), tris.data(), (int)(tris.size() / 3), cell, keep_duplicates);
    write_ply(out_ply, R.xyz.data(), nullptr, (int)(R.xyz.size() / 3), R.triangles.data(), (int)(R.triangles.size() / 3));
    return R;
}

std::vector<float> Mesher::unseen_points(const float* xyz, int nv, const int32_t* tris, int nt, const uint8_t* seen, int n, unsigned long long seed)
{
    std::vector<float> out;
    if (n < 1 || nt < 1 || nv < 1) return out;
    const DevMesh in(xyz, nv, tris, nt);
    DevArr<uint8_t> s((size_t)nv);
    DevArr<float> ov((size_t)nv * 3), pts((size_t)n * 3);
    DevArr<int32_t> ot((size_t)nt * 3);
    s.upload(seen, (size_t)nv);
    int onv = 0, ont = 0;
    check(nsk_mesh_select(ctx(), in.v.p(), nv, in.t.p(), nt, s.p(), 1, ov.p(), ot.p(), nullptr, &onv, &ont, nullptr));
    if (ont == 0) return out;
    double area = 0.0;
    int degenerate = 0;
    check(nsk_mesh_sample(ctx(), ov.p(), onv, ot.p(), ont, seed, n, pts.p(), nullptr, &area, &degenerate));
    out.resize((size_t)n * 3);
    pts.download(out.data(), out.size());
    return out;
}
