/* forwards to the single shim header (see cv_shim.hpp) */
#include "cv_shim.hpp"
