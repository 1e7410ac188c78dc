/* sfmx_ctx_split.h -- context creation in steps.  Exported by libsfmx.so for the host pipeline (libsfmx_host.so); not part of
 * the ABI the Python binding covers (include/sfmx.h).
 *
 * The HIP runtime places a stream on one of its GPU_MAX_HW_QUEUES hardware queues by creation order, and streams that share a
 * queue run their kernels one after the other.  A caller with several contexts that wants their compute streams on different
 * queues therefore has to interleave the stream creations of different contexts (csrc/host/lane_plan.hpp):
 *   sfmx_ctx_create_bare    a context without streams (same arguments and status codes as sfmx_ctx_create_prio);
 *   sfmx_ctx_create_stream  creates one of its two streams, each exactly once (a second call for the same stream is
 *                           SFMX_ERR_INVALID).  The context is usable once it has both.
 * sfmx_ctx_create_prio is sfmx_ctx_create_bare + the copy stream + the compute stream, in that order. */
#ifndef SFMX_CTX_SPLIT_H
#define SFMX_CTX_SPLIT_H

#include "sfmx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SFMX_STREAM_COMPUTE = 0, SFMX_STREAM_COPY = 1 };
int sfmx_ctx_create_bare(int device_id, int priority, sfmx_ctx** out);
int sfmx_ctx_create_stream(sfmx_ctx* ctx, int which);

#ifdef __cplusplus
}
#endif
#endif
