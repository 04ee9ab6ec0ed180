// mcs_rows.hip — mcs_gather_rows / mcs_scatter_rows: rows of an id-indexed device table to and from a list, in units of W bytes.  They take a context and
// touch no store.
#include "mcs_host.h"

namespace mcs {
namespace {

struct FillRow { uint32_t w[64]; };
template <class W>
__global__ __launch_bounds__(256) void k_gather_rows(const int* idx, long long total, int upr, const W* src, FillRow fill, W* dst) {
	const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
	if (t >= total) return;
	const long long i = t / upr;
	const int j = (int)(t - i * upr);
	const int k = idx[i];
	dst[t] = k >= 0 ? src[(long long)k * upr + j] : reinterpret_cast<const W*>(fill.w)[j];
}
template <class W>
__global__ __launch_bounds__(256) void k_scatter_rows(const int* idx, long long total, int upr, const W* src, W* dst) {
	const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
	if (t >= total) return;
	const long long i = t / upr;
	const int j = (int)(t - i * upr);
	const int k = idx[i];
	if (k >= 0) dst[(long long)k * upr + j] = src[t];
}

}  // namespace
}  // namespace mcs

using namespace mcs;

static int row_unit(const void* a, const void* b, int rowBytes) {
	const uintptr_t m = (uintptr_t)a | (uintptr_t)b | (uintptr_t)rowBytes;
	return (m & 15) == 0 ? 16 : (m & 7) == 0 ? 8 : (m & 3) == 0 ? 4 : 1;
}

int mcs_gather_rows(mcs_ctx* c, const int32_t* idx, int n, const void* src, int row_bytes, const void* fill_row, void* dst) {
	if (!c || n < 0 || row_bytes < 1 || (n > 0 && (!idx || !src || !dst))) return fail(MCS_ERR_INVALID, "null argument / bad sizes");
	if (row_bytes > (int)sizeof(FillRow)) return fail(MCS_ERR_UNSUPPORTED, "rows of more than 256 bytes");
	if (n == 0) return MCS_OK;
	HIPCHK(hipSetDevice(c->device));
	FillRow fill;
	memset(&fill, 0, sizeof(fill));
	if (fill_row) memcpy(&fill, fill_row, row_bytes);
	const int u = row_unit(src, dst, row_bytes), upr = row_bytes / u;
	const long long total = (long long)n * upr;
	const dim3 g((unsigned)((total + 255) / 256)), b(256);
	if (u == 16) hipLaunchKernelGGL(k_gather_rows<uint4>, g, b, 0, c->stream, idx, total, upr, (const uint4*)src, fill, (uint4*)dst);
	else if (u == 8) hipLaunchKernelGGL(k_gather_rows<uint2>, g, b, 0, c->stream, idx, total, upr, (const uint2*)src, fill, (uint2*)dst);
	else if (u == 4) hipLaunchKernelGGL(k_gather_rows<uint32_t>, g, b, 0, c->stream, idx, total, upr, (const uint32_t*)src, fill, (uint32_t*)dst);
	else hipLaunchKernelGGL(k_gather_rows<uint8_t>, g, b, 0, c->stream, idx, total, upr, (const uint8_t*)src, fill, (uint8_t*)dst);
	HIPCHK(hipGetLastError());
	return MCS_OK;
}

int mcs_scatter_rows(mcs_ctx* c, const int32_t* idx, int n, const void* src, int row_bytes, void* dst) {
	if (!c || n < 0 || row_bytes < 1 || (n > 0 && (!idx || !src || !dst))) return fail(MCS_ERR_INVALID, "null argument / bad sizes");
	if (n == 0) return MCS_OK;
	HIPCHK(hipSetDevice(c->device));
	const int u = row_unit(src, dst, row_bytes), upr = row_bytes / u;
	const long long total = (long long)n * upr;
	const dim3 g((unsigned)((total + 255) / 256)), b(256);
	if (u == 16) hipLaunchKernelGGL(k_scatter_rows<uint4>, g, b, 0, c->stream, idx, total, upr, (const uint4*)src, (uint4*)dst);
	else if (u == 8) hipLaunchKernelGGL(k_scatter_rows<uint2>, g, b, 0, c->stream, idx, total, upr, (const uint2*)src, (uint2*)dst);
	else if (u == 4) hipLaunchKernelGGL(k_scatter_rows<uint32_t>, g, b, 0, c->stream, idx, total, upr, (const uint32_t*)src, (uint32_t*)dst);
	else hipLaunchKernelGGL(k_scatter_rows<uint8_t>, g, b, 0, c->stream, idx, total, upr, (const uint8_t*)src, (uint8_t*)dst);
	HIPCHK(hipGetLastError());
	return MCS_OK;
}
