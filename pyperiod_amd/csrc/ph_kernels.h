// Kernels of libperiod_hip.so, one header per algorithm.  One workgroup owns one signal window (or one window and a
// slice of the candidate periods); the window is read from HBM once and lives in LDS for the whole algorithm.
// Reference citations are file:line into /root/reference/pyPeriod/.
#pragma once

// (the kernels that are no templates -- the three window-pair kernels and k_dict_project -- reach the code object in
// the order of these lines)
#include "ph_mbest.h"
#include "ph_s2l.h"
#include "ph_bc.h"
#include "ph_bf.h"
#include "ph_ram.h"
#include "ph_qo.h"
#include "ph_project.h"
#include "ph_path.h"
