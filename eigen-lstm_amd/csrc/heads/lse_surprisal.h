// lse_surprisal.h -- the log-sum-exp surprisal shared by the softmax kernels, k_eval_bits and the inference heads.
// Included by kernels.hip inside namespace lstmk, at the place this text stood, and by the host emulations under tests/
// (tests/device_shim.h supplies the device words there).  Not a translation unit of its own.
// LSTM_HIP_STABLE_SOFTMAX: -log2 p_t of p = exp(z - zmax) / s in log-sum-exp form (finite where p_t underflows to 0)
__device__ __forceinline__ float lse_surprisal(float s, float zmax, float zt) {
    return log2f(s) + (zmax - zt) * 1.44269504088896341f;
}
