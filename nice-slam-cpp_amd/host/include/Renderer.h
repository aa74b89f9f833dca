// Same surface as the reference's include/Renderer.h:8-25: constructor, eval_points and render_batch_ray keep their
// signatures (note rays_d before rays_o).  Every call marshals into include/nsk.h.
#pragma once
#include <tuple>
#include <utility>
#include <torch/torch.h>
#include <yaml-cpp/yaml.h>
#include "models/NICE.h"

class Renderer {
  public:
    Renderer();
    // not in the reference (its constants are literals): the constants above, then the keys of the configuration's `rendering:` block that
    // are honoured here -- rendering.N_importance, an absent key or block meaning 0.  The Tracker and the Mapper build their Renderer so.
    explicit Renderer(const YAML::Node& ns_config);
    torch::Tensor eval_points(torch::Tensor p, NICE decoders, c10::Dict<std::string, torch::Tensor> c, std::string stage);
    void render_batch_ray(c10::Dict<std::string, torch::Tensor> c, NICE decoders, torch::Tensor rays_d, torch::Tensor rays_o,
                          std::string stage, torch::Tensor gt_depth, torch::Tensor& rgb_map, torch::Tensor& depth_map,
                          torch::Tensor& depth_var, torch::Tensor& weights);
    // not in the reference (upstream NICE-SLAM's Renderer.render_img): the whole H x W frame seen from c2w ([3][4] or [4][4]) rendered from
    // the map in chunks of ray_batch_size pixels, each chunk a batch of its own with its own max(gt_depth) (src/Renderer.cpp:76,93), so the
    // frame depends on ray_batch_size as it does upstream.  gt_depth [H][W] or an undefined tensor (no ground truth: N_surface = 0).
    // Returns (depth [H][W], uncertainty [H][W], color [H][W][3]).  Rays are generated on the device (nsk_render_image).
    std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> render_img(c10::Dict<std::string, torch::Tensor> c, NICE decoders, torch::Tensor c2w,
                                                                         std::string stage, torch::Tensor gt_depth, int H, int W, float fx,
                                                                         float fy, float cx, float cy);
    // not in the reference (the evaluation of rendered keyframes): structural similarity of two images, [H][W] or [H][W][C] with C <= 4, on
    // the device (nsk_image_ssim with the defaults win 11, sigma 1.5, k1 0.01, k2 0.03; levels = 5: MS-SSIM with the standard weights).
    // Returns (the result: SSIM for levels = 1, else MS-SSIM; the level-0 SSIM).  h_out (or NULL): the call's eight doubles.
    std::pair<double, double> image_ssim(torch::Tensor a, torch::Tensor b, int levels = 1, double data_range = 1.0, double* h_out = nullptr);
    // not in the reference: the scene bound is hard-coded there in five places (src/Renderer.cpp:15 ...)
    void set_bound(torch::Tensor bound_3x2);
    torch::Tensor bound;
    // N_importance (rendering.N_importance through Renderer(ns_config), default 0): extra depths per ray drawn from the compositing weights of a first pass; every
    // renderer that takes this Renderer's constants (render_batch_ray, render_img, the Mapper's, the Tracker's, and the Mesher's calls that
    // follow) then returns the second pass over N_samples (+ N_surface) + N_importance samples (include/nsk.h: nsk_set_importance)
    int N_samples, N_surface, N_importance;
    bool lindisp, occupancy;
    float perturb;

  private:
    void push_opts();
    int points_batch_size, ray_batch_size;
    int scale;
};
