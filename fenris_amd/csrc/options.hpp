#pragma once
// The FENRIS_HIP_* switches of a context as a struct: one member per line of options.def, parsed once (fh_create, fh_set_option) and read
// as c->opt.NAME.  A name options.def does not declare does not compile here and is refused at the boundary.
#include <string>
#include <vector>

namespace fenris_hip_detail {

using OptFLAG = bool;   // the variable is present, whatever its value
struct OptINT {         // atoi of a non-empty value
    bool set = false;
    int value = 0;
    int value_or(int dflt) const { return set ? value : dflt; }
};
struct OptENV_ONLY {};  // read with getenv where it is used; in the table for completeness

struct Options {
#define FH_OPT(name, kind, dflt, doc) Opt##kind name{};
#include "options.def"
#undef FH_OPT
};

enum class OptResult { OK, UNKNOWN, ENV_ONLY };
// Sets (value != nullptr) or clears the switch with this full name ("FENRIS_HIP_...").
OptResult option_set(Options& o, const char* name, const char* value);
// The full name of the index-th switch of options.def; nullptr past the end.
const char* option_name(int index);
// Every FENRIS_HIP_* variable of the environment into o; the names options.def does not know are appended to `unknown`.
void options_from_env(Options& o, std::vector<std::string>& unknown);

}  // namespace fenris_hip_detail
