/* engine_internal.h — C entry points that engine.cpp defines for the library's other translation units (boundary.hip,
 * graph.cpp).  Not part of the public ABI (include/lpmp_engine.h, which also declares lpmp_engine_stream). */
#pragma once
#include "../../include/lpmp_engine.h"

#ifdef __cplusplus
extern "C" {
#endif
int lpmp_set_last_error(const char* msg);      /* the text lpmp_last_error returns on this thread; returns 0 */
int lpmp_boundary_enter(lpmp_engine* e);       /* the engine's device current, speculative passes settled, no aborted chain run behind */
int lpmp_boundary_leave(lpmp_engine* e);       /* duals were written through device offsets */
void* lpmp_engine_dual_base(lpmp_engine* e);   /* the dual base pointer the device offsets are relative to */
int64_t lpmp_engine_device_dual_offset(lpmp_engine* e, int64_t packed_off);       /* a packed dual offset as a device offset (rows layout) */
int lpmp_engine_dual_range_ok(lpmp_engine* e, int64_t packed_off, int64_t len);   /* a run of doubles inside one factor's dual */
#ifdef __cplusplus
}
#endif
