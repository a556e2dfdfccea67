// The switch table of options.def: parsing of one (name, value) pair, the list of names, the walk over the environment.
#include "options.hpp"

#include <cstdlib>
#include <cstring>
#include <utility>

extern char** environ;

namespace fenris_hip_detail {

static const char PREFIX[] = "FENRIS_HIP_";
static const size_t PREFIX_LEN = sizeof PREFIX - 1;

static const char* const NAMES[] = {
#define FH_OPT(name, kind, dflt, doc) "FENRIS_HIP_" #name,
#include "options.def"
#undef FH_OPT
};

static OptResult assign(OptFLAG& m, const char* v) { m = v != nullptr; return OptResult::OK; }
static OptResult assign(OptINT& m, const char* v) {
    m.set = v && *v;
    m.value = m.set ? std::atoi(v) : 0;
    return OptResult::OK;
}
static OptResult assign(OptENV_ONLY&, const char*) { return OptResult::ENV_ONLY; }

OptResult option_set(Options& o, const char* name, const char* value) {
    if (std::strncmp(name, PREFIX, PREFIX_LEN) != 0) return OptResult::UNKNOWN;
    const char* s = name + PREFIX_LEN;
#define FH_OPT(name, kind, dflt, doc) if (std::strcmp(s, #name) == 0) return assign(o.name, value);
#include "options.def"
#undef FH_OPT
    return OptResult::UNKNOWN;
}

const char* option_name(int index) {
    return (index >= 0 && index < (int)(sizeof NAMES / sizeof NAMES[0])) ? NAMES[index] : nullptr;
}

void options_from_env(Options& o, std::vector<std::string>& unknown) {
    for (char** ev = environ; ev && *ev; ++ev) {
        if (std::strncmp(*ev, PREFIX, PREFIX_LEN) != 0) continue;
        const char* eq = std::strchr(*ev, '=');
        if (!eq) continue;
        std::string name(*ev, (size_t)(eq - *ev));
        if (option_set(o, name.c_str(), eq + 1) == OptResult::UNKNOWN) unknown.push_back(std::move(name));
    }
}

}  // namespace fenris_hip_detail
