// fusion.hpp -- the fusion and content-weight entry points that cross translation units
// (input_prep.hip, content_weights.hip; autobbox.hip fuses through them).
#pragma once

#include "common.hpp"

namespace spimdecon {

// content_weights.hip: the sigma rules (SPIMDECON_ERR_ARG) ...
void check_content_sigmas(const double* sigma1, const double* sigma2);

// ... and ContentBased.approximateEntropy on device buffers: img, out and tmp hold dims voxels
// each (img is only read; out receives the weights).  Drains s.
void content_weights_device(const float* img, const int64_t dims[3], const double* sigma1, const double* sigma2,
                            float* out, float* tmp, hipStream_t s);

// input_prep.hip: sigma1 / sigma2 (nviews x 3, both or neither): content-based weights per view
void fuse_weighted_average(int nviews, const spim_view_source* views, const spim_fusion_params* p,
                           const float* borders, const float* ranges, const double* sigma1, const double* sigma2,
                           float* out);

}  // namespace spimdecon
