"""FLAC responses (ev_flac, ev_flac_lpc): the configuration of the device encoder and a file writer.

The encoder itself is HIP (csrc/ev_flac.hip) behind the C entries ev_flac and ev_flac_lpc; include/evhip.h states the stream it writes: 16-bit
mono, a fixed block size, CONSTANT / VERBATIM / FIXED subframes and, with ``max_lpc_order`` > 0, LPC subframes of order 1 .. 12 (Welch window,
Levinson-Durbin in fp64, one precision, no precision search); with ``md5`` the STREAMINFO carries the MD5 of the samples.  The streams have been
held byte for byte to a numpy restatement of that specification and decoded by an independent decoder written from the format (tests/); neither
libFLAC nor ffmpeg has read them.  Nothing here touches the device.
"""
import ctypes as C
from dataclasses import dataclass

SAMPLE_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
BLOCK_SIZES = (256, 512, 1024, 2048, 4096)
CONVERT = {"wrap": 0, "clamp": 1}
KIND_CONSTANT, KIND_VERBATIM, KIND_FIXED = 0, 1, 8      # frame_kind: a FIXED subframe of order o is 8 + o
KIND_LPC = 32                                           # an LPC subframe of order o is 32 + (o - 1)
MAX_LPC_ORDER = 12


@dataclass
class FlacConfig:
    sample_rate: int = 16000
    block_size: int = 4096
    max_fixed_order: int = 4
    max_partition_order: int = 5
    convert: str = "wrap"      # fp32 input only: "wrap" = the bits of wav_float_to_int16 (a pcm response), "clamp" = ev_stitch's int16 rule
    max_lpc_order: int = 0     # 0: no LPC subframes (ev_flac's streams); 1 .. 12: ev_flac_lpc
    qlp_precision: int = 12    # bits of a quantised LPC coefficient, 5 .. 15
    md5: bool = False          # STREAMINFO carries the MD5 of the samples (one serial chain per stream on the device)

    def validate(self) -> "FlacConfig":
        if int(self.sample_rate) not in SAMPLE_RATES:
            raise ValueError("sample_rate %r is not one of %s" % (self.sample_rate, SAMPLE_RATES))
        if int(self.block_size) not in BLOCK_SIZES:
            raise ValueError("block_size %r is not one of %s" % (self.block_size, BLOCK_SIZES))
        if not 0 <= int(self.max_fixed_order) <= 4:
            raise ValueError("max_fixed_order %r outside [0, 4]" % (self.max_fixed_order,))
        if not 0 <= int(self.max_partition_order) <= 6:
            raise ValueError("max_partition_order %r outside [0, 6]" % (self.max_partition_order,))
        if self.convert not in CONVERT:
            raise ValueError("convert %r is neither 'wrap' nor 'clamp'" % (self.convert,))
        if not 0 <= int(self.max_lpc_order) <= MAX_LPC_ORDER:
            raise ValueError("max_lpc_order %r outside [0, %d]" % (self.max_lpc_order, MAX_LPC_ORDER))
        if not 5 <= int(self.qlp_precision) <= 15:
            raise ValueError("qlp_precision %r outside [5, 15]" % (self.qlp_precision,))
        if not isinstance(self.md5, (bool, int)) or int(self.md5) not in (0, 1):
            raise ValueError("md5 %r is neither False nor True" % (self.md5,))
        return self

    def to_ext(self):
        """The ev_flac_ext of ev_flac_lpc, or None for the identity case (no LPC, no MD5): the call is then ev_flac itself."""
        if int(self.max_lpc_order) == 0 and not self.md5:
            return None
        from . import _ffi
        e = _ffi.ev_flac_ext()
        e.struct_size = C.sizeof(_ffi.ev_flac_ext)
        e.max_lpc_order, e.qlp_precision, e.md5 = int(self.max_lpc_order), int(self.qlp_precision), int(bool(self.md5))
        return e

    def to_struct(self):
        from . import _ffi
        c = _ffi.ev_flac_config()
        c.struct_size = C.sizeof(_ffi.ev_flac_config)
        c.sample_rate, c.block_size = int(self.sample_rate), int(self.block_size)
        c.max_fixed_order, c.max_partition_order, c.convert = int(self.max_fixed_order), int(self.max_partition_order), CONVERT[self.convert]
        return c


def flac_bound(n: int, block_size: int = 4096) -> int:
    """ev_flac_bound: the largest stream a segment of n samples can give (host only)."""
    from . import _ffi
    v = int(_ffi.lib().ev_flac_bound(int(n), int(block_size)))
    if v < 0:
        raise ValueError("flac_bound: n = %r or block_size = %r out of range" % (n, block_size))
    return v


def write_flac(path: str, data: bytes) -> None:
    """Writes one stream as ev_flac made it.  Anything that is not a FLAC stream is refused: an array would need the device encoder."""
    if not isinstance(data, (bytes, bytearray, memoryview)) or bytes(data[:4]) != b"fLaC":
        raise ValueError("write_flac takes the bytes of a stream from EVEngine.flac / synthesize(..., flac=True), not samples")
    with open(path, "wb") as f:
        f.write(data)
