// host_options.h — the bodies of the estimator options' mod_set_* / mod_get_* functions (EstimatorOptions, mod_context.h), shared by the files that
// own an option: host_sgm.hip, host_flow.hip, host_filters.hip.  One setter and one getter: field, check (int (ModContext *, const T &)), default.
#pragma once
#include "mod_context.h"

// v == null: back to the default; a failed check leaves the stored value as it was
template <class T, class Check>
int set_option(ModContext *c, T EstimatorOptions::*field, const T *v, Check check) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (int rc = v ? check(c, *v) : MOD_OK) return rc;
  c->opt.*field = v ? *v : EstimatorOptions{}.*field;
  return MOD_OK;
}
template <class T>
int get_option(const ModContext *c, T EstimatorOptions::*field, T *out) {
  if (!c || !out) return MOD_ERR_INVALID_ARGUMENT;
  *out = c->opt.*field;
  return MOD_OK;
}
