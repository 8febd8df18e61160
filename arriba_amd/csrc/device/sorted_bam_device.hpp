// sorted_bam_device.hpp -- what the kernels that write stored BGZF blocks share (agpu_sorted_bam.hip: sorted_bam_gather_kernel; agpu_supporting.hip: support_pool_copy_kernel,
// supporting_gather_kernel): the copy of a run of bytes by one wavefront (destination-aligned words, the source read with aligned words and shifts, ragged ends by bytes), and
// the frame of a block around a payload that lies in LDS (tables and header bytes in front, CRC-32 from LDS, trailer, 16-byte stores behind; the compressing gather of
// agpu_sorted_bam.hip takes the CRC and the stores by themselves).  Device code only.
#ifndef AGPU_SORTED_BAM_DEVICE_HPP
#define AGPU_SORTED_BAM_DEVICE_HPP 1

#include <hip/hip_runtime.h>
#include "crc32_core.hpp"
#include "sorted_bam_core.hpp"

namespace agpu {

const int SBAM_GATHER_THREADS = 1024;     // 16 wavefronts: one record each at a time
const uint32_t SBAM_IMAGE_BYTES = (SBAM_BLOCK + 15 + 15) / 16 * 16; // the block as it lies in memory, shifted by the alignment of its first byte (0 .. 15)
const uint32_t SBAM_CRC_LANE_BYTES = 64, SBAM_CRC_VIRTUAL_BYTES = SBAM_CRC_LANE_BYTES * SBAM_GATHER_THREADS; // the payload is the END of a virtual block of 64 KiB whose front is zero bytes (crc32_core.hpp)
const uint32_t SBAM_CRC_SERIAL_BELOW = 64; // a payload this short (the tail of a file) is done by one lane
static_assert(SBAM_CRC_VIRTUAL_BYTES >= SBAM_PAYLOAD, "the virtual block holds a payload");

// One wavefront: stream[source .. source + (end - at)) -> destination[at .. end).  `destination` is 4-byte aligned (an LDS image, or a buffer of hipMalloc); every word read
// from the stream holds a byte of the run.
template <class Offset> __device__ __forceinline__ void sbam_wave_copy(uint8_t* destination, Offset at, Offset end, const uint8_t* stream, uint64_t source, uint32_t lane) {
	uint32_t head = (4 - (uint32_t) (at & 3u)) & 3u;
	if (head > end - at) head = (uint32_t) (end - at);
	if (lane < head) destination[at + lane] = stream[source + lane];
	const Offset words = (end - at - head) / 4; const uint32_t tail = (uint32_t) ((end - at - head) & 3u);
	uint32_t* const destination_words = (uint32_t*) destination;
	for (Offset k = lane; k < words; k += 64) destination_words[(at + head) / 4 + k] = sbam_load32(stream, source + head + 4ull * k); // (aligned words of the stream and a shift: every word read holds a byte of the record)
	if (lane < tail) destination[end - tail + lane] = stream[source + (end - at) - tail + lane];
}

struct SbamFrameShared {
	uint4 image[SBAM_IMAGE_BYTES / 16];
	uint32_t crc_byte_table[256];
	uint32_t advance[CRC32_ADVANCE_POWERS][32];
};

// the tables of the CRC into LDS, the 23 bytes in front of a payload of `length` bytes into the image (image byte pad + i is byte i of the block).  No barrier inside.
__device__ __forceinline__ void sbam_frame_begin(SbamFrameShared& shared, const Crc32Tables* __restrict__ tables, uint32_t pad, uint32_t length, uint32_t t) {
	uint8_t* const image = (uint8_t*) shared.image;
	if (t < 256) shared.crc_byte_table[t] = tables->slice[0][t];
	for (uint32_t k = t; k < CRC32_ADVANCE_POWERS * 32; k += SBAM_GATHER_THREADS) shared.advance[k / 32][k % 32] = tables->advance[k / 32][k % 32];
	if (t < SBAM_HEAD) image[pad + t] = sbam_head_byte(t, length);
}

// Behind a barrier that follows the last write of the payload: the CRC-32 of image[payload_at .. payload_at + length) taken from LDS (64 bytes per lane, joined pairwise);
// every lane gets it, behind a barrier.  `partial`: SBAM_GATHER_THREADS words of LDS.  All SBAM_GATHER_THREADS lanes of the workgroup call it.
__device__ __forceinline__ uint32_t sbam_frame_crc(SbamFrameShared& shared, uint32_t* partial, uint32_t payload_at, uint32_t length, uint32_t t) {
	uint8_t* const image = (uint8_t*) shared.image;
	if (length < SBAM_CRC_SERIAL_BELOW) {
		if (t == 0) partial[0] = ~crc32_of(shared.crc_byte_table, image + payload_at, length);
	} else {
		// raw CRCs (register started at 0) of the 64-byte chunks of the virtual block: zero bytes in front change nothing, and the standard start is the first four bytes inverted
		const int32_t shift = (int32_t) (SBAM_CRC_VIRTUAL_BYTES - length);
		uint32_t c = 0;
		const int32_t chunk = (int32_t) (t * SBAM_CRC_LANE_BYTES) - shift; // where the chunk begins in the payload
		if (chunk + (int32_t) SBAM_CRC_LANE_BYTES > 0) {
			for (int32_t i = chunk < 0 ? -chunk : 0; i < (int32_t) SBAM_CRC_LANE_BYTES; ++i) {
				const int32_t m = chunk + i;
				uint32_t byte = image[payload_at + m];
				if (m < 4) byte ^= 0xFFu;
				c = shared.crc_byte_table[(c ^ byte) & 0xFFu] ^ (c >> 8);
			}
		}
		partial[t] = c;
		for (uint32_t level = 0, stride = 1; stride < SBAM_GATHER_THREADS; ++level, stride *= 2) { // crc(A || B) = crc(A) advanced over |B| zero bytes, xor crc(B); |B| = 64 << level
			__syncthreads();
			if (t % (2 * stride) == 0) partial[t] = gf2_matrix_times(shared.advance[6 + level], partial[t]) ^ partial[t + stride];
		}
	}
	__syncthreads();
	return ~partial[0];
}

// image[pad .. pad + size) stored to block_out (pad = block_out & 15): whole 16-byte chunks of memory with one store each, the ragged ends byte by byte (the neighbours' bytes of
// those chunks are theirs).  Behind a barrier that follows the last write of the image.
__device__ __forceinline__ void sbam_frame_store(SbamFrameShared& shared, uint32_t pad, uint32_t size, uint8_t* block_out, uint32_t t) {
	uint8_t* const image = (uint8_t*) shared.image;
	const uint32_t image_end = pad + size;
	const uint32_t first_chunk = (pad + 15) / 16, end_chunk = image_end / 16;
	uint4* const aligned_out = (uint4*) (block_out - pad);
	for (uint32_t chunk = first_chunk + t; chunk < end_chunk; chunk += SBAM_GATHER_THREADS) aligned_out[chunk] = shared.image[chunk];
	const uint32_t head_end = first_chunk * 16 < image_end ? first_chunk * 16 : image_end;
	if (pad + t < head_end) block_out[t] = image[pad + t];
	const uint32_t tail_begin = end_chunk * 16 > head_end ? end_chunk * 16 : head_end;
	if (tail_begin + t < image_end) block_out[tail_begin + t - pad] = image[tail_begin + t];
}

// Behind a barrier that follows the last write of the payload: the CRC-32 of the payload, the trailer, and the stored block to block_out
__device__ __forceinline__ void sbam_frame_finish(SbamFrameShared& shared, uint32_t* partial, uint32_t pad, uint32_t length, uint8_t* block_out, uint32_t t) {
	uint8_t* const image = (uint8_t*) shared.image;
	const uint32_t payload_at = pad + SBAM_HEAD;
	const uint32_t crc = sbam_frame_crc(shared, partial, payload_at, length, t);
	if (t < SBAM_TAIL) image[payload_at + length + t] = sbam_tail_byte(t, crc, length);
	__syncthreads();
	sbam_frame_store(shared, pad, length + SBAM_HEAD + SBAM_TAIL, block_out, t);
}

}

#endif
