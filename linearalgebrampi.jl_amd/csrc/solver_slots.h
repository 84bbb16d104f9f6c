// solver_slots.h -- slots of the MINRES solver's scalar buffer (include/hpcla_rocm.h): the kernels in vecops.hip read and
// write them, the iterations loop in solvers.hip points the SpMV's dot at MINRES_YT.  Library-internal.
#pragma once

namespace hpcla {

enum MinresSlot {
    MINRES_BETA = 0, MINRES_OLDB = 1, MINRES_YT = 2, MINRES_BB = 3, MINRES_ALFA = 4, MINRES_CS = 5, MINRES_SN = 6, MINRES_DBAR = 7,
    MINRES_EPSLN = 8, MINRES_OLDEPS = 9, MINRES_DELTA = 10, MINRES_GBAR = 11, MINRES_GAMMA = 12, MINRES_PHI = 13,
    MINRES_PHIBAR = 14, MINRES_SCALARS = 16
};

}  // namespace hpcla
