/* forwards to the single shim header (see cv_shim.hpp) */
#include <sstream>   /* Thirdparty/DBoW2's TemplatedVocabulary.h uses std::stringstream and includes only this */
#include "cv_shim.hpp"
