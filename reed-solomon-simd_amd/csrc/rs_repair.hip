// Column kernels of a repair (rs_repair_device*): the decode's kernel body with a
// second destination map over the recovery rows (rs_device.hpp MonoArgs2,
// launch_mono_repair / launch_mono_half_repair), and the batch repair with one
// pattern per stripe (MonoMaskArgs2, launch_mono_repair_masks).
//
// The body is rs_mono.hip's; this translation unit builds only its repair
// instantiations (k_mono_repair, k_mono_repair_masks), rs_mono.hip's own object none of them, so the
// decode's kernels and their arguments stay as they were and the two objects
// compile in parallel.
#define RS_MONO_REPAIR_TU 1
#include "rs_mono.hip"
