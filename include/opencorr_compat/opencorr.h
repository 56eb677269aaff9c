// opencorr.h -- umbrella header of the MI355X drop-in for OpenCorr's FFTCC -> ICGN path
// (the reference's umbrella is src/opencorr.h:20-42; the hot-path classes and the stereo chain exist here).
#pragma once
#include "oc_deformation.h"
#include "oc_engines.h"
#include "oc_feature_affine.h"
#include "oc_feature_detect.h"
#include "oc_feature_match.h"
#include "oc_io.h"
#include "oc_stereo.h"
#include "oc_types.h"
