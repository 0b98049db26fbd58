// Stand-in header: everything lives in arvx_ref_cv.hpp (see there).
#include "../arvx_ref_cv.hpp"
