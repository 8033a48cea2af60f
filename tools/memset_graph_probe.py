"""Does this HIP runtime replay a captured hipMemsetAsync node faithfully?  ("Every slot is written".)

One valid device buffer per case and nothing else: the memset is captured alone into a graph on one stream, the buffer is refilled
with 0xA5 before every replay, and from the third replay on a device-to-device copy of an unrelated buffer runs in between.  Prints,
per (size, value), how many 32-bit words are wrong after each replay.  When every line says 0, ewn_playout_wins and
ewn_endgame_build could clear with hipMemsetAsync again (k_zero_wins, k_endgame_clear), and tests/test_gpu_stream_contract.py's
property (a) would confirm it.

    python tools/memset_graph_probe.py
"""
import ctypes

import torch


def main():
    path = [line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line][0]     # the runtime torch has loaded
    hip = ctypes.CDLL(path)
    print("runtime: %s, torch %s, hip %s" % (path, torch.__version__, torch.version.hip))
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    fill = -1515870811        # 0xA5A5A5A5
    for nbytes, value in ((1200, 0), (1200, 7), (4096, 0), (1 << 20, 0)):
        x = torch.zeros(nbytes // 4, dtype=torch.int32, device="cuda")
        y, z = torch.zeros(100000, device="cuda"), torch.ones(100000, device="cuda")
        want = int.from_bytes(bytes([value]) * 4, "little", signed=True)
        x.fill_(fill)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="global"):
            rc = hip.hipMemsetAsync(x.data_ptr(), value, nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        print("%d bytes of value %d: rc %d, ran during the capture: %s" % (nbytes, value, rc, bool((x != fill).any())))
        for i in range(4):
            x.fill_(fill)
            if i >= 2:
                y.copy_(z)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            print("  replay %d: %d of %d words wrong, first words %s" % (
                i + 1, int((x != want).sum()), x.numel(), [hex(v & 0xFFFFFFFF) for v in x[:4].tolist()]))


if __name__ == "__main__":
    main()
