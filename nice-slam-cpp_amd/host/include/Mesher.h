// Mesher.h -- the scene mesh.  The reference's config/nice_slam.yaml:16-26 carries a `meshing:` block and mapping.mesh_freq, and the
// reference ships no class that reads them; this one reads
//   meshing.resolution (256)   nodes per axis of the lattice.  The lattice spans the bound enlarged by `padding` on every side, first
//                              node on bound.lo - padding, last node on bound.hi + padding, so the step along an axis is
//                              (extent + 2 padding) / (resolution - 1): `resolution` counts NODES, not cells, on the longest and the
//                              shortest axis alike (cells are not cubes unless the bound is);
//   meshing.level_set (0)      the occupancy level of the surface (inside = occupancy above it);
// and leaves clean_mesh (frustum-hull culling), mesh_coarse_level, get_largest_components, remove_small_geometry_threshold and the
// render_ray_query colouring to the caller.  Points outside the bound have occupancy 100 (src/Renderer.cpp:36): with padding > 0 the
// bound's own faces therefore show up as a shell around the scene, with padding 0 the outermost nodes (which lie ON the open bound) do.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include <torch/torch.h>
#include <yaml-cpp/yaml.h>
#include "models/NICE.h"

class Mesher {
  public:
    Mesher(YAML::Node ns_config, torch::Tensor bound_3x2 = torch::Tensor(), float padding = 0.f);
    void set_bound(torch::Tensor bound_3x2);
    // nsk_eval_lattice (fine) -> nsk_mesh_extract -> (color) nsk_eval_points (color) on the device vertex buffer, rgb clamped to [0, 1] -> PLY.
    // valid: optional uint8 / bool [resolution^3] (z, y, x order), 0 = cells touching the node are skipped.
    void get_mesh(const std::string& path, NICE& decoders, c10::Dict<std::string, torch::Tensor> c, bool color = true,
                  torch::Tensor valid = torch::Tensor());
    // binary little-endian PLY: float x y z, (rgb given) uchar red green blue, list uchar int vertex_indices
    static void write_ply(const std::string& path, const float* xyz, const uint8_t* rgb, int n_vertices, const int32_t* triangles, int n_triangles);
    static void read_ply(const std::string& path, std::vector<float>& xyz, std::vector<uint8_t>& rgb, std::vector<int32_t>& triangles);

    int resolution;
    float level_set, padding;
    torch::Tensor bound;
    int last_vertices = 0, last_triangles = 0;
};
