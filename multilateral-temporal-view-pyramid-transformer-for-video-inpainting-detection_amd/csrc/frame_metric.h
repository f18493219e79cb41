// frame_metric.h — the per-frame F1 / IoU of the four counts {inter, sum p, sum g, union} in fp64 (measure.py:57-62, 86-89 as
// mumpy_hip.distributed.eval_metric_vector states them): frame_metrics_kernel (video_stage.hip) applies it to the counts of one
// threshold, sweep_metrics_kernel (score_sweep.hip) to the counts of every threshold of a table.  One definition for both.
#pragma once
#include "common.h"

namespace mumpy {

// eps_g = 1e-6 * npix: measure.py sums (gt + 1e-6) over all pixels
__device__ __forceinline__ void frame_f1_iou(double inter, double sp, double sg, double uni, double eps_g, double& f1, double& iou) {
    const double recall = inter / (sg + eps_g);
    const double precision = inter / (sp + 1e-6);
    f1 = 2.0 * precision * recall / (precision + recall + 1e-6);
    iou = (inter + 1e-5) / (uni + 1e-5);
}

}  // namespace mumpy
