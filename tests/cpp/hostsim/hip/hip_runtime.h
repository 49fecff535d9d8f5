// Stand-in for <hip/hip_runtime.h>, for building csrc/hgi_capi.hip with plain g++ against the simulated runtime of
// tests/cpp/hostsim/hostsim.cpp (profiles/r16_host_routes.md).  Only what the host layer behind include/hgi.h uses, with the
// names, values and signatures of HIP's public API.  Test code: nothing under rustyhgi_amd/ includes this file.
#pragma once
#include <stddef.h>
#include <stdint.h>

typedef enum hipError_t {
    hipSuccess = 0,
    hipErrorInvalidValue = 1,
    hipErrorOutOfMemory = 2,
    hipErrorInvalidResourceHandle = 400,
    hipErrorNotReady = 600
} hipError_t;

typedef enum hipMemcpyKind {
    hipMemcpyHostToHost = 0,
    hipMemcpyHostToDevice = 1,
    hipMemcpyDeviceToHost = 2,
    hipMemcpyDeviceToDevice = 3,
    hipMemcpyDefault = 4
} hipMemcpyKind;

typedef enum hipStreamCaptureStatus {
    hipStreamCaptureStatusNone = 0,
    hipStreamCaptureStatusActive,
    hipStreamCaptureStatusInvalidated
} hipStreamCaptureStatus;

typedef struct ihipStream_t *hipStream_t;
typedef struct ihipEvent_t *hipEvent_t;

#define hipStreamDefault 0x00
#define hipStreamNonBlocking 0x01
#define hipEventDefault 0x0
#define hipEventDisableTiming 0x2
#define hipHostMallocDefault 0x0
#define hipHostRegisterDefault 0x0

extern "C" {
hipError_t hipGetDeviceCount(int *count);
hipError_t hipSetDevice(int device);
hipError_t hipGetLastError(void);
const char *hipGetErrorString(hipError_t e);

hipError_t hipMalloc(void **ptr, size_t size);
hipError_t hipFree(void *ptr);
hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int flags);
hipError_t hipHostFree(void *ptr);
hipError_t hipHostRegister(void *ptr, size_t size, unsigned int flags);
hipError_t hipHostUnregister(void *ptr);

hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned int flags);
hipError_t hipStreamDestroy(hipStream_t stream);
hipError_t hipStreamSynchronize(hipStream_t stream);
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned int flags);
hipError_t hipStreamIsCapturing(hipStream_t stream, hipStreamCaptureStatus *status);

hipError_t hipEventCreate(hipEvent_t *event);
hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned int flags);
hipError_t hipEventDestroy(hipEvent_t event);
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream);
hipError_t hipEventSynchronize(hipEvent_t event);
hipError_t hipEventElapsedTime(float *ms, hipEvent_t start, hipEvent_t stop);

hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream);
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind,
                            hipStream_t stream);
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t stream);
}
