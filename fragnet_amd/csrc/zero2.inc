// k_zero2_i32: zeroes two int32 ranges in one launch (a kernel, not a memset: the same node kind in a captured graph as everything around
// it).  Included into the anonymous namespace of the units that launch it -- batch_io.hip, head.hip, param_grads.hip -- and of no other:
// a __global__ function that is no template is compiled into every unit that sees it, launched or not.
__global__ void k_zero2_i32(int32_t* __restrict__ a, int64_t na, int32_t* __restrict__ b, int64_t nb) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < na) a[i] = 0;
        else b[i - na] = 0;
    }
}
