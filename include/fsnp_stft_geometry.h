/*
 * fsnp_stft_geometry.h - the STFT geometry of a handle's waveform path.  Part of the public surface of libfsnp_hip.so next to
 * fsnp.h (which includes this header), same FSNP_ABI_VERSION.  DESIGN.md (f-3, "STFT geometry") has the kernels' side.
 *
 * The reference reads n_fft, hop_length and win_length from [acoustics] of its TOML and hands them to torch.stft / torch.istft
 * (audio_zen/acoustics/feature.py:10-56).  What of that is free here:
 *
 *   n_fft       = 2 (num_freqs - 1), for any num_freqs >= 3: a one-sided spectrum of num_freqs bins leaves no other choice.
 *   win_length  = n_fft, periodic Hann: the reference's wrapper builds hann_window(n_fft), and torch refuses a window of another size.
 *   hop_length  the free parameter, n_fft / 8 <= hop_length <= n_fft / 2 and hop_length % 4 == 0; it need not divide n_fft.
 *               The default is n_fft / 2 = num_freqs - 1.
 *
 * Why these bounds.  Above n_fft / 2 no frame covers the clip's last samples for some lengths (torch.istft pads them with zeros);
 * below n_fft / 8 nobody runs an enhancer.  The frames of the forward DFT GEMM are read where they lie in the padded signal, row t
 * at float t * hop_length, as 16-byte vectors: hence hop_length % 4.  n_fft itself is under no such rule: the rows of the DFT
 * matrices are padded to what the GEMM reads (a multiple of 16 floats), and the frame rows of a wave session to a multiple of 4.
 *
 * fsnp_stft, fsnp_istft, fsnp_enhance_wave, fsnp_enhance_wave_lengths, fsnp_reserve(max_samples > 0), fsnp_wave_stream_create and
 * fsnp_wave_stream_create_live read the handle's geometry when they are called: T = 1 + samples / hop_length frames per clip, reflect
 * padding of n_fft / 2 samples (so a clip needs more than n_fft / 2 samples whatever the hop).  A wave session keeps the hop it was
 * created with; a later fsnp_set_hop_length does not touch it.  The DFT matrices depend on n_fft only and survive a change of the hop.
 * Spectrum and mag sessions know no hop: their caller owns the STFT.
 */
#ifndef FSNP_STFT_GEOMETRY_H
#define FSNP_STFT_GEOMETRY_H

#include "fsnp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sets the hop of the handle's waveform path.  Host arithmetic only: no GPU call, nothing is enqueued.  Code 1: null handle.  Code 2,
 * with the rule that was broken: hop_length outside [n_fft / 8, n_fft / 2] (n_fft / 8 rounded up) or not a multiple of 4. */
int fsnp_set_hop_length(fsnp_handle* h, int32_t hop_length);
/* The hop in force (num_freqs - 1 until fsnp_set_hop_length); 0 for a null handle. */
int32_t fsnp_hop_length(const fsnp_handle* h);

#ifdef __cplusplus
}
#endif

#endif /* FSNP_STFT_GEOMETRY_H */
