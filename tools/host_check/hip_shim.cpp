// hip_shim.cpp -- a stand-in for the HIP runtime on a machine without a GPU, for checking the HOST code of libpyclaw_amd
// under a sanitizer (tools/host_check/run.sh).  "Device" memory is host memory from calloc, copies are memcpy, so a host
// copy that is too long for either side is an out-of-bounds access the sanitizer sees.  Kernels do not run: a launch is a
// no-op, except that a launch of ONE thread is taken for the Courant-number hand-over (pclaw.hip: cfl_handover(word, host,
// seq)) and carried out, so that a step of a 1-D or 3-D solver returns (with Courant number 0 and q unchanged).
// Only the entry points the library's objects reference are here.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>

namespace {
struct Config { dim3 grid, block; size_t shmem; hipStream_t stream; } g_cfg;
void *handle() { return malloc(1); }
}  // namespace

extern "C" {

void **__hipRegisterFatBinary(const void *) { static void *h = nullptr; return &h; }
void __hipRegisterFunction(void **, const void *, char *, const char *, unsigned, void *, void *, void *, void *, int *) {}
void __hipUnregisterFatBinary(void **) {}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
    g_cfg = {grid, block, shmem, stream};
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *shmem, hipStream_t *stream) {
    *grid = g_cfg.grid, *block = g_cfg.block, *shmem = g_cfg.shmem, *stream = g_cfg.stream;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void *, dim3 grid, dim3 block, void **args, size_t, hipStream_t) {
    if (grid.x * grid.y * grid.z * block.x * block.y * block.z == 1) {
        unsigned long long *word = *(unsigned long long **)args[0], *host = *(unsigned long long **)args[1];
        host[0] = *word;
        *word = 0;
        __atomic_store_n(host + 1, *(unsigned long long *)args[2], __ATOMIC_RELEASE);
    }
    return hipSuccess;
}

hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "hip_shim"; }

hipError_t hipMalloc(void **p, size_t n) { *p = calloc(n ? n : 1, 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void *p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return hipMalloc(p, n); }
hipError_t hipHostFree(void *p) { free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned) { *d = h; return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }

hipError_t hipDeviceGetStreamPriorityRange(int *lo, int *hi) { *lo = 0, *hi = 0; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)handle(); return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int) { *s = (hipStream_t)handle(); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)handle(); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)handle(); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.0f; return hipSuccess; }

hipError_t hipModuleLoadData(hipModule_t *, const void *) { return hipErrorNotSupported; }
hipError_t hipModuleGetFunction(hipFunction_t *, hipModule_t, const char *) { return hipErrorNotSupported; }
hipError_t hipModuleUnload(hipModule_t) { return hipErrorNotSupported; }
hipError_t hipModuleLaunchKernel(hipFunction_t, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, hipStream_t,
                                 void **, void **) { return hipErrorNotSupported; }

}  // extern "C"
