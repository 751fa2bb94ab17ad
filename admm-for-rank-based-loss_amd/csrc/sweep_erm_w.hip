// sweep_erm_w.hip - the row-weighted twins (SE_FUSED_W) of the single-sweep erm kernels, in a translation unit of their
// own: sweep_erm.hip compiled a second time for launch_sweep_erm_w alone.  Every fused instance has a twin (three losses,
// three storage types), so one unit with both would be what the whole build waits for.
#define RBL_SWEEP_ERM_W_UNIT 1
#include "sweep_erm.hip"
