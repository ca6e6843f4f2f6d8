// The option table of pyslam_amd/csrc/ps_options.h behind a C interface, for tests/test_options_host.py (ctypes).
#include "ps_options.h"

extern "C" {
int opt_count(void) { return PS_NUM_OPTIONS; }
const char* opt_name(int i) { return PS_OPTION_TABLE[i].name; }
int opt_size(void) { return (int)sizeof(PsOptions); }
void opt_fresh(PsOptions* o) { *o = PsOptions{}; }
int opt_apply(PsOptions* o, const char* name, double value, const char** refusal) { return ps_option_apply(*o, name, value, refusal); }
int opt_codes(void) { return (-PS_OPT_UNKNOWN) | (-PS_OPT_REFUSED) << 4; }
int opt_effect_bits(void) { return PS_FX_COARSE_REBUILD | PS_FX_DROP_FACTOR << 4 | PS_FX_DROP_SIDE << 8 | PS_FX_RELOOK_PATH << 12 | PS_FX_LDI_OFF << 16; }
// the member(s) behind a name; "ldi_direct" as the option's own three values: 1 on, -1 allowed but not on, 0 not allowed
double opt_get(const PsOptions* o, const char* name) {
    const PsOptionRow* r = ps_option_find(name);
    if (!r) return NAN;
    if (r->kind == PS_OPT_SPIN) return o->cp_spin;
    if (r->kind == PS_OPT_COST_TOL) return o->ldi_cost_tol;
    if (r->kind == PS_OPT_LDI_DIRECT) return o->ldi_direct ? 1 : (o->ldi_direct_ok ? -1 : 0);
    return o->*r->member;
}
int opt_ldi_possible(const PsOptions* o, long n) { return ps_ldi_possible(*o, n); }
}
