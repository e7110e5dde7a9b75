// Thread-local last-error string for the C ABI (mt_last_error()).
#include <stdarg.h>
#include <stdio.h>

#include "mt_common.h"

namespace mt {
static thread_local char g_err[1024] = {0};
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* last_error() { return g_err; }

// the calling thread's current output-store policy (mt_common.h)
static thread_local int g_store_policy = 0;
int store_policy() { return g_store_policy; }
StorePolicyScope::StorePolicyScope(int policy) : prev_(g_store_policy) { g_store_policy = policy; }
StorePolicyScope::~StorePolicyScope() { g_store_policy = prev_; }
void StorePolicyScope::set(int policy) { g_store_policy = policy; }
}  // namespace mt
