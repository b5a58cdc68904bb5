// The engine parameters OpticalFlowOpenCV runs a frame size with; OpticalFlowBank configures its engine by the same
// function, so that a bank of S streams computes what S OpticalFlowOpenCV objects compute.  Not installed.
#pragma once

#include "aof.h"
#include "flow_opencv.hpp"
#include "flow_px4.hpp"

inline void opencvEngineParams(int img_width, int img_height, int num_feat, aof_params *out)
{
	aof_params p;
	aof_params_px4flow(&p, img_width, img_height, DEFAULT_SEARCH_SIZE, DEFAULT_FLOW_FEATURE_THRESHOLD,
			   DEFAULT_FLOW_VALUE_THRESHOLD);
	int per_axis = 1;
	while (per_axis * per_axis < num_feat) per_axis++;
	p.num_blocks = per_axis;
	// The class mainloop.cpp:423 creates runs at 128x128 and ~75 Hz on a moving vehicle: a
	// single +-4 search would pin fast motion at the search limit while still reporting a
	// plausible quality.  Two levels with per-level mean equalisation reach +-9.5 px and
	// shrug off the auto-exposure steps; geometries that cannot carry a half-resolution grid
	// keep the single level (getPyramidLevels() says which).
	aof_params two = p;
	two.pyramid_levels = 2;
	two.mean_subtract = 1;
	*out = aof_params_check(&two) == 0 ? two : p;
}
