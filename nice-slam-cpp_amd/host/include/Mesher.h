// Mesher.h -- the scene mesh.  The reference's config/nice_slam.yaml:16-26 carries a `meshing:` block and mapping.mesh_freq, and the
// reference ships no class that reads them; this one reads
//   meshing.resolution (256)   nodes per axis of the lattice.  The lattice spans the bound enlarged by `padding` on every side, first
//                              node on bound.lo - padding, last node on bound.hi + padding, so the step along an axis is
//                              (extent + 2 padding) / (resolution - 1): `resolution` counts NODES, not cells, on the longest and the
//                              shortest axis alike (cells are not cubes unless the bound is);
//   meshing.level_set (0)      the occupancy level of the surface (inside = occupancy above it);
//   meshing.remove_small_geometry_threshold (0.2), meshing.get_largest_components (false)   get_clean_mesh only: components of the mesh
//                              with less surface than the threshold (m^2) are dropped, or all but the largest;
//   meshing.color_mesh_extraction_method (direct_point_query)   how a vertex gets its colour: direct_point_query decodes the colour at the
//                              vertex; render_ray_along_normal renders the colour stage along a ray of color_ray_length (0.1 m, upstream's
//                              constant) that looks at the vertex from free space along its normal (nsk_mesh_vertex_normals,
//                              nsk_mesh_vertex_colors), and decodes at the vertex where it has no normal.  Any other value throws;
//   meshing.clean_mesh_bound_scale (1.02)   get_hull_mesh only: upstream's get_mesh bound.  The keyframes' depth is fused (as in
//                              get_fused_mesh), the convex hull of the fusion's vertices and the camera centres is taken on the device
//                              (nsk_points_hull), scaled about its centre by this factor, and the map is evaluated and meshed at the lattice
//                              nodes inside it (nsk_lattice_in_hull).  get_clean_mesh culls per node with the union of the keyframes'
//                              depth-truncated frusta instead: tighter, and with holes wherever nothing was observed;
// and leaves mesh_coarse_level to the caller.  Points outside the bound have occupancy 100 (src/Renderer.cpp:36): with padding > 0 the
// bound's own faces therefore show up as a shell around the scene, with padding 0 the outermost nodes (which lie ON the open bound) do.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include <torch/torch.h>
#include <yaml-cpp/yaml.h>
#include "models/NICE.h"

// upstream's three 3D numbers of a reconstruction against a ground-truth mesh (src/tools/eval_recon.py) and what went into them
struct ReconMetrics {
    double accuracy_cm = 0, completion_cm = 0, completion_ratio_pct = 0;      // mean rec -> gt, mean gt -> rec, share of gt samples below the threshold
    double accuracy_max_cm = 0, completion_max_cm = 0;
    double rec_area = 0, gt_area = 0;                                         // m^2, degenerate triangles left out
    int rec_degenerate = 0, gt_degenerate = 0;                                // triangles without an area or with an index out of range
    int rec_skipped = 0, gt_skipped = 0;                                      // samples with a non-finite coordinate left out of the targets
    double transform[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // align: the reconstruction was measured under this (row-major 4x4)
    double icp_fitness = 0, icp_rmse = 0;                                     // align: share of rec vertices with a gt vertex within reach, their rmse (m)
    int icp_iterations = 0;                                                   // align: updates applied
    // surface: the samples were measured against the other MESH (nsk_mesh_nearest), not against its samples; rec_skipped / gt_skipped then
    // count the triangles left out
    bool surface = false;
    double precision_pct = 0, recall_pct = 0, fscore_pct = 0;                 // rec samples below the threshold, = completion_ratio_pct, 2PR / (P + R) (0 when P + R is 0)
    double normal_accuracy = 0, normal_completion = 0, normal_consistency = 0;        // mean |cos| of a sample's own triangle and the nearest one, each way, and their mean
    int normal_skipped = 0;                                                   // pairs without two normals (nsk_normal_stats)
};

// upstream's 2D number of a reconstruction, Depth L1 (src/tools/eval_recon.py calc_2d_metric), and what went into it
struct ReconDepth {
    double depth_l1_cm = 0;                 // 100 x the mean over the used views of sum |gt - rec| / n_pix (background zeros included, as upstream)
    double restricted_l1_cm = 0;            // 100 x sum |gt - rec| / count over the pixels of the used views where both meshes are hit
    int n_views = 0, n_used = 0;            // views drawn; views whose ground-truth cover reaches min_cover
    int rec_skipped = 0, gt_skipped = 0;    // triangles with an index out of range
    std::vector<double> view_l1, view_cover;        // per view: sum |gt - rec| / n_pix (m), the share of pixels the ground truth covers
    std::vector<double> stats;              // [n_views][4]: nsk_depth_pair_stats(gt, rec)
    std::vector<float> w2c;                 // [n_views][16]: the views (nsk_depth_views)
    int candidates_tried = 0;               // with unseen points: candidates of the view stream looked at (n_views is then the accepted number)
    std::vector<long long> view_index;      // with unseen points: the accepted candidates' indices in the stream
    double transform[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};     // align: as in ReconMetrics
    double icp_fitness = 0, icp_rmse = 0;
    int icp_iterations = 0;
};

// what Mesher::align_recon found (nsk_cloud_icp's h_M and h_info)
struct ReconAlign {
    double transform[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int iterations = 0, correspondences = 0;
    double fitness = 0, rmse = 0;
    bool converged = false, degenerate = false;
};

// what Mesher::cull_mesh returns: the part of a mesh a trajectory saw
struct CulledMesh {
    std::vector<float> xyz;                 // [vertices][3]: the vertices a kept triangle names, in their old order
    std::vector<int32_t> triangles;         // [triangles][3]: the triangles whose three vertices were seen, re-indexed, in their old order
    std::vector<int32_t> vertex_src;        // [vertices]: the input index of every output vertex
    std::vector<uint8_t> seen;              // [input vertices]: 1 = at least one frame saw it
    long long n_seen = 0;                   // set bytes of seen
    int skipped = 0;                        // triangles with an index out of range (in neither part)
};

// what Mesher::simplify_mesh returns: the mesh clustered on a uniform grid (nsk_mesh_simplify)
struct SimplifiedMesh {
    std::vector<float> xyz;                 // [vertices][3]: one representative per cell a kept triangle names, in ascending cell index
    std::vector<int32_t> triangles;         // [triangles][3]: the triangles that are neither collapsed nor duplicates, re-indexed, in their old order
    std::vector<int32_t> vertex_map;        // [input vertices]: the output vertex of every input vertex, or -1
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // nsk_mesh_simplify's h_info: finite, left out, invalid, collapsed, duplicates, occupied cells, cells, packed dimensions
};

class Mesher {
  public:
    Mesher(YAML::Node ns_config, torch::Tensor bound_3x2 = torch::Tensor(), float padding = 0.f);
    void set_bound(torch::Tensor bound_3x2);
    // nsk_eval_lattice (fine) -> nsk_mesh_extract -> (color) nsk_mesh_vertex_colors on the device vertex buffer by color_method, rgb clamped to
    // [0, 1] -> PLY.  get_mesh, get_clean_mesh, get_fused_mesh and get_rendered_mesh all write the context's mesh the same way: color_method,
    // color_ray_length and write_normals hold for each of them, and the normals are those of the mesh that is written (after the filter).
    // valid: optional uint8 / bool [resolution^3] (z, y, x order), 0 = cells touching the node are skipped; the lattice is then evaluated at
    // the set nodes only (nsk_eval_lattice_masked, fill 100), which leaves the mesh unchanged.
    void get_mesh(const std::string& path, NICE& decoders, c10::Dict<std::string, torch::Tensor> c, bool color = true,
                  torch::Tensor valid = torch::Tensor());
    // The mesh of what the keyframes saw: nsk_lattice_seen on the lattice of get_mesh over the keyframes in batches of at most 16 (depths: host
    // tensors [H, W] of metric z-depth, 0 / NaN / inf = no measurement; c2ws: [4, 4] camera-to-world, camera looking along -z, inverted in
    // double) -> nsk_eval_lattice_masked (fine) at the seen nodes, 100 elsewhere -> nsk_mesh_extract with that mask -> nsk_mesh_filter
    // (remove_small_geometry_threshold / get_largest_components) -> colour query on the filtered vertices -> PLY.  Lattice, mask and mesh
    // stay on the device.
    void get_clean_mesh(const std::string& path, NICE& decoders, c10::Dict<std::string, torch::Tensor> c, const std::vector<torch::Tensor>& depths,
                        const std::vector<torch::Tensor>& c2ws, int H, int W, float fx, float fy, float cx, float cy, bool color = true);
    // The mesh of what the sensor measured: the depth frames (depths: host tensors [H, W] of metric z-depth, 0 / NaN / inf = no
    // measurement; c2ws: [4, 4] camera-to-world, camera looking along -z, inverted in double) fused into a truncated signed distance
    // volume on the lattice of get_mesh (resolution, padding, bound) by nsk_tsdf_integrate, 32 frames' images on the device at a time,
    // truncation trunc_steps times the largest step (3: this project's first choice) -> nsk_tsdf_volume (min_weight) ->
    // nsk_mesh_extract at level 0 -> nsk_mesh_filter when remove_small_geometry_threshold > 0 or get_largest_components -> PLY without
    // colours.  Needs no map: the comparison mesh for eval_recon / eval_recon_depth / cull_mesh where the dataset ships none.
    void get_fused_mesh(const std::string& path, const std::vector<torch::Tensor>& depths, const std::vector<torch::Tensor>& c2ws, int H, int W,
                        float fx, float fy, float cx, float cy, float trunc_steps = 3.f, float min_weight = 1.f);
    // The mesh of what the map renders: the same over the depth that nsk_render_image renders at every pose (stage; the sensor depth
    // depths[k] guides the sampling as in Renderer::render_img, an empty depths vector renders without guidance; chunks of chunk_rays
    // pixels; the render options are the context's, i.e. those of the last Renderer call).  The rendered frames stay on the device.
    // Colours come from the colour query on the vertex buffer, as in get_mesh.
    void get_rendered_mesh(const std::string& path, NICE& decoders, c10::Dict<std::string, torch::Tensor> c, const std::vector<torch::Tensor>& depths,
                           const std::vector<torch::Tensor>& c2ws, int H, int W, float fx, float fy, float cx, float cy, float trunc_steps = 3.f,
                           float min_weight = 1.f, bool color = true, const std::string& stage = "color", int chunk_rays = 25600);
    // Upstream's Mesher.get_mesh: the room, including the parts no camera saw but the map fills in, without the shell the bound's faces
    // and the untrained corners of the grids leave around it.  The frames are fused on the lattice of get_mesh as in get_fused_mesh (no
    // component filter); nsk_points_hull takes the hull of the fused vertices, still in the context's device buffer, and the camera centres
    // c2w[:3, 3]; nsk_lattice_in_hull marks the nodes inside the hull scaled by clean_mesh_bound_scale; nsk_eval_lattice_masked (fine)
    // decodes at those nodes, 100 elsewhere; nsk_mesh_extract runs WITH the mask.  So, like get_clean_mesh and unlike upstream's
    // z[~mask] = 100, no shell is drawn along the hull: a surface that crosses it ends there.  Colours, normals and the PLY as in get_mesh.
    // Without a hull (fewer than four points in general position) the mesh is empty.  hull_from_context: the fusion and the hull are
    // skipped and the hull the context holds is taken (nsk_hull_upload: a caller's own convex bound).
    void get_hull_mesh(const std::string& path, NICE& decoders, c10::Dict<std::string, torch::Tensor> c, const std::vector<torch::Tensor>& depths,
                       const std::vector<torch::Tensor>& c2ws, int H, int W, float fx, float fy, float cx, float cy, bool color = true,
                       float trunc_steps = 3.f, float min_weight = 1.f);
    // binary little-endian PLY: float x y z, (rgb given) uchar red green blue, list uchar int vertex_indices
    static void write_ply(const std::string& path, const float* xyz, const uint8_t* rgb, int n_vertices, const int32_t* triangles, int n_triangles);
    static void read_ply(const std::string& path, std::vector<float>& xyz, std::vector<uint8_t>& rgb, std::vector<int32_t>& triangles);
    // the same with vertex normals (or nullptr: the file of the function above, byte for byte): float x y z, float nx ny nz, (rgb given) uchar
    // red green blue, in this order; and its reader (normals / rgb come back empty when the file has none)
    static void write_ply(const std::string& path, const float* xyz, const float* normals, const uint8_t* rgb, int n_vertices, const int32_t* triangles,
                          int n_triangles);
    static void read_ply(const std::string& path, std::vector<float>& xyz, std::vector<float>& normals, std::vector<uint8_t>& rgb,
                         std::vector<int32_t>& triangles);
    // Any PLY mesh, read by its header: format ascii or binary_little_endian; the vertex element's x, y, z found by name among scalar
    // properties of any type, number and order and converted to float; the face element's first list property with any count and index
    // type, polygons of more than three corners fan-triangulated (0, k, k + 1), faces of fewer than three dropped; every other element and
    // property skipped.  Throws std::runtime_error carrying the path: big-endian, a malformed header, a truncated file, an index out of range.
    static void read_ply_mesh(const std::string& path, std::vector<float>& xyz, std::vector<int32_t>& triangles);
    // Accuracy / completion / completion ratio on the device: n_points area-weighted samples of each mesh (nsk_mesh_sample with seed and
    // seed + 1), exact nearest distances both ways (nsk_cloud_nearest), the sums (nsk_cloud_stats).  Coordinates in metres; the meshes
    // are taken as they are: callers that follow upstream's protocol pass meshes culled by cull_mesh.  With align the reconstruction's vertices are first registered to the ground truth's
    // (align_recon) and the transformed mesh is measured.  With surface the rec samples are measured against the gt mesh and the gt samples
    // against the rec mesh (nsk_mesh_nearest: exact point-to-triangle distances), and precision / recall / F-score and the normal
    // consistency (nsk_normal_stats on each sample's own triangle and the nearest one) are filled in as well.  A static function: it needs
    // no map, only the process's context.
    static ReconMetrics eval_recon(const std::string& rec_ply, const std::string& gt_ply, int n_points = 200000, float threshold = 0.05f,
                                   unsigned long long seed = 0, bool align = false, bool surface = false);
    static ReconMetrics eval_recon(const float* rec_xyz, int rec_vertices, const int32_t* rec_triangles, int rec_n_triangles, const float* gt_xyz,
                                   int gt_vertices, const int32_t* gt_triangles, int gt_n_triangles, int n_points = 200000,
                                   float threshold = 0.05f, unsigned long long seed = 0, bool align = false, bool surface = false);
    // upstream's get_align_transformation: point-to-point ICP of the reconstruction's vertices onto the ground truth's from the identity
    // (nsk_cloud_icp: Open3D's registration_icp, relative fitness / rmse 1e-6).  Host arrays [n][3]; nothing is changed.
    static ReconAlign align_recon(const float* rec_xyz, int rec_vertices, const float* gt_xyz, int gt_vertices, float threshold = 0.1f,
                                  int max_iter = 30);
    // Depth L1 on the device: n_views random views inside the ground truth's box (nsk_depth_views: seed, shrink), both meshes rendered as
    // H x W depth images with fx = fy = focal, cx = W / 2 - 0.5, cy = H / 2 - 0.5 (nsk_mesh_depth) in batches that keep both stacks below
    // about 1 GB, the per-view sums (nsk_depth_pair_stats).  A view is used when the ground truth covers at least min_cover of its pixels
    // (0: every view, upstream's plain mean).  With align the reconstruction is registered first, as in eval_recon.  With unseen_xyz
    // ([n_unseen][3], host: the never-observed ground truth, unseen_points) the views are the first n_views candidates of the same stream
    // that have none of those points in their image (nsk_depth_views_range + nsk_points_view_counts in rounds of 32, at most
    // 16 n_views candidates): upstream's redraw.  n_views of the result is then the number accepted (it may be smaller).
    static ReconDepth eval_recon_depth(const std::string& rec_ply, const std::string& gt_ply, int n_views = 1000, int H = 500, int W = 500,
                                       float focal = 300.f, unsigned long long seed = 0, double shrink = 0.7, double min_cover = 0.0,
                                       bool align = false);
    static ReconDepth eval_recon_depth(const float* rec_xyz, int rec_vertices, const int32_t* rec_triangles, int rec_n_triangles,
                                       const float* gt_xyz, int gt_vertices, const int32_t* gt_triangles, int gt_n_triangles,
                                       int n_views = 1000, int H = 500, int W = 500, float focal = 300.f, unsigned long long seed = 0,
                                       double shrink = 0.7, double min_cover = 0.0, bool align = false, const float* unseen_xyz = nullptr,
                                       int n_unseen = 0);
    // upstream's cull_mesh.py on the device: the part of a mesh the trajectory w2c ([K][16] row-major world-to-camera, host; the camera
    // looks along -z) saw, per vertex by the rule of nsk_points_seen, then nsk_mesh_select (part 0).
    //   occlusion "none": the view frusta alone;  "depth": against the sensor depth images depths ([K][H][W], host), a pixel without a
    //   measurement sees nothing;  "self": every batch of frames is rendered from the mesh itself (nsk_mesh_depth) and tested against that.
    // At most frames_per_batch frames' images are on the device at a time; the result does not depend on it.  eps (m): how far behind the
    // depth a vertex still counts as seen; 0.03 is this project's first choice, not upstream's number.
    static CulledMesh cull_mesh(const float* xyz, int n_vertices, const int32_t* triangles, int n_triangles, const float* w2c, int K, int H, int W,
                                float fx, float fy, float cx, float cy, const float* depths = nullptr, const std::string& occlusion = "none",
                                int edge = 0, float eps = 0.03f, int frames_per_batch = 32);
    // the same from a PLY file (read_ply_mesh) into a PLY file (write_ply, no colours)
    static CulledMesh cull_mesh(const std::string& in_ply, const std::string& out_ply, const float* w2c, int K, int H, int W, float fx, float fy,
                                float cx, float cy, const float* depths = nullptr, const std::string& occlusion = "none", int edge = 0,
                                float eps = 0.03f, int frames_per_batch = 32);
    // Uniform vertex clustering on the device (nsk_mesh_simplify, include/nsk.h states the rule): all vertices in one cell of a grid of
    // edge `cell` (m) collapse to their fixed-point mean; collapsed triangles go, and unless keep_duplicates so do triangles that repeat an
    // earlier one's cells in the same cyclic order; vertices no kept triangle names go.  Host arrays; needs no map.
    static SimplifiedMesh simplify_mesh(const float* xyz, int n_vertices, const int32_t* triangles, int n_triangles, float cell,
                                        bool keep_duplicates = false);
    // the same from a PLY file (read_ply_mesh) into a PLY file (write_ply, no colours)
    static SimplifiedMesh simplify_mesh(const std::string& in_ply, const std::string& out_ply, float cell, bool keep_duplicates = false);
    // n area-weighted samples [n][3] of the part of the mesh that was not seen (nsk_mesh_select part 1, then nsk_mesh_sample): what
    // eval_recon_depth takes as unseen_xyz.  Empty when n = 0 or every valid triangle was seen.
    static std::vector<float> unseen_points(const float* xyz, int n_vertices, const int32_t* triangles, int n_triangles, const uint8_t* seen,
                                            int n, unsigned long long seed = 0);

    int resolution;
    float level_set, padding;
    torch::Tensor bound;
    float remove_small_geometry_threshold;
    bool get_largest_components;
    std::string color_method;           // meshing.color_mesh_extraction_method: "direct_point_query" or "render_ray_along_normal"
    float color_ray_length = 0.1f;      // render_ray_along_normal: the ray starts this far (m) out along the normal (upstream's constant)
    bool write_normals = false;         // the PLY carries nx ny nz (nsk_mesh_vertex_normals on the mesh that is written)
    int last_color_fallback = 0;        // vertices coloured by the point query (all of them with direct_point_query)
    int last_normals_zero = 0;          // vertices without a normal (0 when no normals were computed)
    float seen_trunc = 0.5f;    // a node counts as seen up to this far (m) behind the measured depth: the margin inside which the Mapper's own
                                // frustum selection lets voxels train (nsk_frustum_mask)
    int seen_edge = 0;          // pixels ignored along the image border
    int last_vertices = 0, last_triangles = 0;
    // The cell edge (m) of the vertex clustering that get_mesh, get_clean_mesh, get_fused_mesh, get_rendered_mesh and get_hull_mesh apply
    // to the mesh behind the component filter and in front of colours and normals, which are then those of the mesh that is written.
    // 0: off, every PLY is what it is without this member.  last_vertices / last_triangles stay the counts in front of the clustering.
    float simplify_cell = 0.f;
    int last_simplified_vertices = 0, last_simplified_triangles = 0;      // what was written (= last_vertices / last_triangles with simplify_cell 0)
    int last_collapsed = 0, last_duplicates = 0;                          // triangles the clustering dropped
    int last_components = 0, last_kept = 0;     // get_clean_mesh: components before the filter, components kept
    long long last_seen = 0;                    // get_clean_mesh: lattice nodes at least one keyframe saw
    long long last_evaluated = 0;               // lattice nodes the decoders ran on (get_mesh without valid: all of them)
    long long last_observed = 0, last_valid = 0; // get_fused_mesh / get_rendered_mesh: nodes with a weight > 0, nodes with weight >= min_weight
    float clean_mesh_bound_scale;               // meshing.clean_mesh_bound_scale (1.02): get_hull_mesh scales the hull about its centre by it
    bool hull_from_context = false;             // get_hull_mesh: take the hull the context holds instead of fusing the frames
    std::vector<int32_t> last_hull_vertices;    // get_hull_mesh: the hull's vertices, ascending indices into (fused vertices, then camera centres)
    std::vector<int32_t> last_hull_faces;       // [faces][3], wound outwards
    long long last_inside = 0;                  // lattice nodes inside the scaled hull
    float fuse_max_weight = 64.f;               // the weight cap of the fusion (a running mean over at most this many frames)
};
