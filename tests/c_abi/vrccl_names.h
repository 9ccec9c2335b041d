/* vrccl_names.h — the names of the in-process RCCL stand-in (vrccl.hip, test infrastructure).
 *
 * Force-included (-include) in front of both translation units of libedt_comm_virtual.so: the
 * unmodified csrc/edt_comm.cpp and the stand-in. Every nccl* function edt_comm.cpp uses is renamed
 * before <rccl/rccl.h> declares it, so the calls in that file bind to the stand-in's definitions
 * inside the library and no nccl* name is exported (the test process has the real librccl mapped
 * through torch). vrccl.map keeps the renamed symbols local as well.
 */
#ifndef EDT_VRCCL_NAMES_H
#define EDT_VRCCL_NAMES_H

#define ncclGetUniqueId edt_vrccl_impl_GetUniqueId
#define ncclCommInitRank edt_vrccl_impl_CommInitRank
#define ncclCommDestroy edt_vrccl_impl_CommDestroy
#define ncclCommAbort edt_vrccl_impl_CommAbort
#define ncclCommGetAsyncError edt_vrccl_impl_CommGetAsyncError
#define ncclGetErrorString edt_vrccl_impl_GetErrorString
#define ncclReduceScatter edt_vrccl_impl_ReduceScatter
#define ncclAllGather edt_vrccl_impl_AllGather
#define ncclAllToAll edt_vrccl_impl_AllToAll
#define ncclSend edt_vrccl_impl_Send
#define ncclRecv edt_vrccl_impl_Recv
#define ncclGroupStart edt_vrccl_impl_GroupStart
#define ncclGroupEnd edt_vrccl_impl_GroupEnd

#ifdef __cplusplus
extern "C" {
#endif

/* The stand-in's control functions: the only exports of the library besides include/edt_comm.h.
 *   edt_vrccl_set_wait_bound   every host wait of the stand-in (joining a world, a rendezvous) gives
 *                              up after this many seconds and marks its world broken; default 30.
 *                              Returns the previous bound, or a negative value for seconds <= 0.
 *   edt_vrccl_wait_bound       the bound in force.
 *   edt_vrccl_break_world      mark the world of this id (edt_comm_unique_id's bytes) broken: every
 *                              rank waiting in it returns an error at once, every later call fails.
 *                              For a rank that fails before it holds a communicator. 0, or -1 if no
 *                              such world is live.
 *   edt_vrccl_live_worlds      worlds that still have a communicator open.
 *   edt_vrccl_staged_moves     collectives' data movements that went through the temporary so far
 *                              (buffers overlapping across ranks), process-wide.
 *   edt_vrccl_arrivals         times a rank entered a rendezvous so far, process-wide: unchanged
 *                              over a call that was refused before any collective.
 *   edt_vrccl_last_error       this thread's last message from the stand-in. */
double edt_vrccl_set_wait_bound(double seconds);
double edt_vrccl_wait_bound(void);
int edt_vrccl_break_world(const void* id);
int edt_vrccl_live_worlds(void);
unsigned long long edt_vrccl_staged_moves(void);
unsigned long long edt_vrccl_arrivals(void);
const char* edt_vrccl_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* EDT_VRCCL_NAMES_H */
