// The library's tuning / test switches (vsx_set_option; initial values from the environment).  The table, with every option's
// name, environment variable, default and meaning, is in options.cpp.
#pragma once

namespace vsxg {

// current value of option `name`; 0 for a name the table does not hold
long gemm_option(const char* name);

}  // namespace vsxg
