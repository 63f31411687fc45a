// range-v3 name over the shim (see ../detail/shim.hpp); test infrastructure only.
#pragma once
#include "../detail/shim.hpp"
