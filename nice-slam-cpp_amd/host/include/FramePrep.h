// nskh::FramePrep -- what upstream NICE-SLAM's dataset layer does to a frame before the Tracker sees it (src/utils/datasets.py __getitem__:
// cv2.undistort, cv2.resize to the depth size, F.interpolate to cam.crop_size, cam.crop_edge cut off, the intrinsics moved along), on the
// device through nsk_frame_prepare (include/nsk.h states the rule).  Not in the reference: its readers hand out the files' pixels.
//   cam:  H W fx fy cx cy (for the depth image), optional crop_edge, crop_size: [H, W], distortion: [k1, k2, p1, p2[, k3[, k4, k5, k6]]],
//         png_depth_scale, scale
#pragma once
#include <memory>
#include <utility>
#include <opencv2/core.hpp>
#include <yaml-cpp/yaml.h>
#include "nsk_host.h"

namespace nskh {

class FramePrep {
  public:
    explicit FramePrep(const YAML::Node& cam);
    // a crop_size, a distortion or a crop_edge > 0: the frames need preparing (otherwise prepare() is the conversion alone)
    bool active() const { return opts.n_dist > 0 || opts.crop_H > 0 || opts.crop_edge > 0; }
    // raw_rgb CV_8UC3 (channel order kept), raw_depth CV_16UC1 -> (colour [H, W, 3], depth [H, W]): float32 CPU tensors, the form
    // Tracker::run and Mapper::run take.  The raw bytes go up, the prepared floats come back; H, W, fx .. cy and last_border follow.
    std::pair<torch::Tensor, torch::Tensor> prepare(const cv::Mat& raw_rgb, const cv::Mat& raw_depth);
    nsk_frame_opts opts;               // what the cam block said; png_depth_scale is 1 when the block has none (has_png_depth_scale)
    bool has_png_depth_scale = false;
    int H = 0, W = 0;                  // of the prepared frame, for colour and depth images of the cam block's H x W (prepare() updates them)
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f;
    int last_border = 0;               // n_border of the last prepare(): colour pixels that read outside the distorted image
  private:
    int Hd, Wd;
    struct Dev;                        // the raw frame and the prepared one on the device
    std::shared_ptr<Dev> dev;
};

}  // namespace nskh
