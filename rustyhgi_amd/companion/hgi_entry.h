// What the HIP units of the companion libraries share: the error text of the calling thread.  Each library gets a copy of its
// own (nothing here is exported, nothing is linked in common).
// Stateless like its users: no environment, no allocation, no context.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "../../include/hgi.h"

namespace hgi {

// what <lib>_last_error() returns: the text of the calling thread's last refusal
inline thread_local char g_err[512] = "";

__attribute__((format(printf, 2, 3))) inline hgi_status fail(hgi_status st, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return st;
}

}  // namespace hgi
