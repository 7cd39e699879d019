// ubench.inc - included at the end of vdl2hip.hip.  vdl2hip_debug_ubench(): the rates the channeliser's roofline line quotes beside
// its own time - what back-to-back FMAs reach, what a random 16-byte LUT gather costs the CU's LDS pipe, what the channeliser's
// sample loop in miniature runs at, and the shader clock itself - measured on the spot, in a few tens of milliseconds, so that
// bench.py reports this run's numbers and not constants typed in from an earlier profile.  Not declared in vdl2hip.h (a
// measurement hook like the other vdl2hip_debug_* calls); the kernels follow dev/gpu_ubench_clock.hip.
namespace ub {
typedef float v2f __attribute__((ext_vector_type(2)));
struct Clk { unsigned long long core, real; };

template<int PK>
__global__ __launch_bounds__(256) void k_fma(float *out, int iters, float s, Clk *clk) {
	v2f a[8];
	for(int i = 0; i < 8; i++) a[i] = v2f{(float)threadIdx.x + i, (float)i};
	const v2f m = v2f{s, s}, c = v2f{0.5f, 0.25f};
	const unsigned long long t0 = __builtin_readcyclecounter(), r0 = wall_clock64();
	for(int it = 0; it < iters; it++) {
		#pragma unroll
		for(int i = 0; i < 8; i++) {
			if(PK) a[i] = __builtin_elementwise_fma(a[i], m, c);
			else {
				float x = a[i].x, y = a[i].y;
				asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x) : "v"(s), "v"(c.x));
				asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(y) : "v"(s), "v"(c.y));
				a[i].x = x; a[i].y = y;
			}
		}
	}
	const unsigned long long t1 = __builtin_readcyclecounter(), r1 = wall_clock64();
	float r = 0.f;
	for(int i = 0; i < 8; i++) r += a[i].x + a[i].y;
	out[blockIdx.x * 256 + threadIdx.x] = r;
	if(blockIdx.x == 0 && threadIdx.x == 0) { clk->core = t1 - t0; clk->real = r1 - r0; }
}

// the channeliser's sample loop in miniature: per channel-sample one LUT gather (GATHER) or none, the interpolation, the complex mix
// and the two tap sums as packed FP32, the phase add; four "channels" per wavefront share the sample
template<int GATHER>
__global__ __launch_bounds__(256, 4) void k_mix(float *out, int iters, unsigned step, const float *taps, Clk *clk) {
	__shared__ float4 lut[256];
	lut[threadIdx.x] = make_float4(0.001f * (float)threadIdx.x, 1.f, 1e-6f, 2e-6f);
	__syncthreads();
	const int lane = threadIdx.x & 63;
	constexpr int CR = 4;
	unsigned ph[CR], dph[CR];
	for(int c = 0; c < CR; c++) { ph[c] = (unsigned)lane * 2654435761u + c * 977u; dph[c] = step * (2 * c + 1) + 12345u; }
	v2f A0[CR], A1[CR];
	for(int c = 0; c < CR; c++) { A0[c] = v2f{0.f, 0.f}; A1[c] = v2f{0.f, 0.f}; }
	float xr = 0.25f + lane * 1e-3f, xi = -0.125f;
	const float4 e0 = lut[lane];
	const unsigned long long t0 = __builtin_readcyclecounter(), r0 = wall_clock64();
	for(int it = 0; it < iters; it++) {
		#pragma unroll 5
		for(int j = 0; j < 20; j++) {
			const float g0 = taps[j], g1 = taps[20 + j];
			const v2f X = v2f{xr, xi}, Xr = v2f{-xi, xr};
			#pragma unroll
			for(int c = 0; c < CR; c++) {
				const unsigned p = ph[c];
				const float F = (float)(p & 0xffffu);
				float4 e = e0;
				if(GATHER) e = lut[(p >> 16) & 0xffu];
				else asm volatile("" : "+v"(e.x), "+v"(e.y), "+v"(e.z), "+v"(e.w));
				const v2f sc = __builtin_elementwise_fma(v2f{e.z, e.w}, v2f{F, F}, v2f{e.x, e.y});
				const v2f m = __builtin_elementwise_fma(v2f{sc.y, sc.y}, X, v2f{sc.x, sc.x} * Xr);
				A0[c] = __builtin_elementwise_fma(v2f{g0, g0}, m, A0[c]);
				A1[c] = __builtin_elementwise_fma(v2f{g1, g1}, m, A1[c]);
				ph[c] = p + dph[c];
			}
			xr += 1e-6f; xi -= 1e-6f;
		}
	}
	const unsigned long long t1 = __builtin_readcyclecounter(), r1 = wall_clock64();
	float r = 0.f;
	for(int c = 0; c < CR; c++) r += A0[c].x + A0[c].y + A1[c].x + A1[c].y;
	out[blockIdx.x * 256 + threadIdx.x] = r;
	if(blockIdx.x == 0 && threadIdx.x == 0) { clk->core = t1 - t0; clk->real = r1 - r0; }
}

// 16 bytes per lane from a 4 KiB LDS table at pseudo-random entries (ds_read_b128), the access pattern of the channeliser's NCO look-up
__global__ __launch_bounds__(256, 4) void k_lutgather(float *out, int iters, Clk *clk) {
	__shared__ __align__(16) float4 lut[256];
	lut[threadIdx.x] = make_float4((float)threadIdx.x, 1.f, 2.f, 3.f);
	__syncthreads();
	unsigned p = (unsigned)(blockIdx.x * 256 + threadIdx.x) * 2654435761u;
	const unsigned dp = 63913u * (2 * (threadIdx.x & 63) + 1) * 40u + 12345u;
	float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
	const unsigned long long t0 = __builtin_readcyclecounter(), r0 = wall_clock64();
	for(int it = 0; it < iters; it++) {
		#pragma unroll
		for(int i = 0; i < 12; i++) {
			const float4 e = lut[(p >> 16) & 0xffu];
			acc.x += e.x; acc.y += e.y; acc.z += e.z; acc.w += e.w;
			p += dp;
		}
	}
	const unsigned long long t1 = __builtin_readcyclecounter(), r1 = wall_clock64();
	out[blockIdx.x * 256 + threadIdx.x] = acc.x + acc.y + acc.z + acc.w;
	if(blockIdx.x == 0 && threadIdx.x == 0) { clk->core = t1 - t0; clk->real = r1 - r0; }
}

// `launch` back to back for >= warm_ms (the shader clock idles low and takes tens of ms of load to come up), then 5 timed launches.
// Returns ms per launch; *mhz = wave 0's shader clocks over its 100 MHz real-time clocks
// (-1: a launch, an event or the copy failed - the warm-up loop also ends after 4096 launches whatever the clock says)
template<typename F> static double timed(F launch, float warm_ms, hipEvent_t e0, hipEvent_t e1, Clk *dclk, double *mhz, double *core_per_launch) {
	float ms = 0.f;
	if(hipEventRecord(e0, nullptr) != hipSuccess) return -1.0;
	int n = 0;
	do {
		launch();
		if(hipGetLastError() != hipSuccess || hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1.0;
	} while(ms < warm_ms && ++n < 4096);
	if(hipEventRecord(e0, nullptr) != hipSuccess) return -1.0;
	for(int i = 0; i < 5; i++) launch();
	if(hipGetLastError() != hipSuccess || hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1.0;
	Clk h{}; if(hipMemcpy(&h, dclk, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
	if(mhz) *mhz = h.real ? (double)h.core / ((double)h.real / 100.0) : 0.0;
	if(core_per_launch) *core_per_launch = (double)h.core;
	return ms / 5.0;
}
}  // namespace ub

extern "C" {
// out[0] v_fma_f32 TFLOP/s   out[1] v_pk_fma_f32 TFLOP/s   out[2] shader clock, MHz (under the FMA load)
// out[3] shader clocks per random 16-byte wave-gather and CU (LDS)
// out[4] shader clocks per channel-sample and wave of the channeliser's sample loop in miniature, with its LUT gather   out[5] without (VALU only)
// out[6] compute units used for the conversions   out[7] milliseconds the measurement took
int vdl2hip_debug_ubench(int device, double out[8]) {
	if(!out) return VDL2HIP_E_INVAL;
	// the caller's current device is put back on every way out (and the buffers and events below release themselves)
	struct Scope { int prev = -1; ~Scope() { if(prev >= 0) (void)hipSetDevice(prev); } } sc;
	if(hipGetDevice(&sc.prev) != hipSuccess) sc.prev = -1;
	HIPCHK(hipSetDevice(device));
	hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, device));
	const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	DevBuf<float> o, taps; DevBuf<ub::Clk> dclk; Event e0, e1, ea, eb;
	HIPCHK(o.alloc((size_t)cus * 8 * 256)); HIPCHK(taps.alloc(40)); HIPCHK(dclk.alloc(1));
	for(Event *e : { &e0, &e1, &ea, &eb }) HIPCHK(e->ensure());
	float h_taps[40]; for(int i = 0; i < 40; i++) h_taps[i] = 0.01f * (float)(i + 1);
	HIPCHK(hipMemcpy(taps, h_taps, sizeof h_taps, hipMemcpyHostToDevice));
	HIPCHK(hipEventRecord(ea, nullptr));
	const int grid = cus * 4;                                        // 4 workgroups of 4 waves per CU = 4 waves per SIMD, one round
	double mhz = 0.0, core = 0.0;
	{
		const int iters = 4096; const double flops = (double)grid * 256 * iters * 16 * 2;
		double ms = ub::timed([&] { hipLaunchKernelGGL(ub::k_fma<0>, dim3(grid), dim3(256), 0, nullptr, o, iters, 1.0001f, dclk); }, 40.f, e0, e1, dclk, &mhz, nullptr);
		if(ms <= 0.0) return VDL2HIP_E_DEVICE;
		out[0] = flops / ms / 1e9; out[2] = mhz;
		ms = ub::timed([&] { hipLaunchKernelGGL(ub::k_fma<1>, dim3(grid), dim3(256), 0, nullptr, o, iters, 1.0001f, dclk); }, 10.f, e0, e1, dclk, nullptr, nullptr);
		if(ms <= 0.0) return VDL2HIP_E_DEVICE;
		out[1] = flops / ms / 1e9;
	}
	{
		const int it3 = 1024; const double gathers = (double)it3 * 12;
		const double ms = ub::timed([&] { hipLaunchKernelGGL(ub::k_lutgather, dim3(grid), dim3(256), 0, nullptr, o, it3, dclk); }, 10.f, e0, e1, dclk, &mhz, nullptr);
		if(ms <= 0.0) return VDL2HIP_E_DEVICE;
		out[3] = ms * 1e-3 * mhz * 1e6 / (16.0 * gathers);            // 16 waves per CU share its one LDS pipe
	}
	{
		const int it2 = 512; const double cs = (double)it2 * 20 * 4;      // channel-samples per wave
		if(ub::timed([&] { hipLaunchKernelGGL(ub::k_mix<1>, dim3(grid), dim3(256), 0, nullptr, o, it2, 40u * 63913u, (const float *)taps, dclk); }, 10.f, e0, e1, dclk, nullptr, &core) <= 0.0) return VDL2HIP_E_DEVICE;
		out[4] = core / cs;
		if(ub::timed([&] { hipLaunchKernelGGL(ub::k_mix<0>, dim3(grid), dim3(256), 0, nullptr, o, it2, 40u * 63913u, (const float *)taps, dclk); }, 10.f, e0, e1, dclk, nullptr, &core) <= 0.0) return VDL2HIP_E_DEVICE;
		out[5] = core / cs;
	}
	HIPCHK(hipEventRecord(eb, nullptr)); HIPCHK(hipEventSynchronize(eb));
	float total = 0.f; (void)hipEventElapsedTime(&total, ea, eb);
	out[6] = cus; out[7] = total;
	return VDL2HIP_OK;
}
}  // extern "C"
