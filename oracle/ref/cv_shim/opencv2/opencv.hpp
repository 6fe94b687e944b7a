/* forwards to the single shim header (see cv_shim.hpp); include/Sim3Solver.h and include/Initializer.h include this one */
#include "cv_shim.hpp"
