"""What the native engines compute, as one SHA-256 per case: the logits of one `forward_prepared` on every geometry of tests/unet_cases.py and on the small
shipped configurations of oracle/golden_configs.py, and `decode_indices` / `encode` of the two tiny VQGANs -- in both precision modes, and for the UNets once
more after perturbed weights were reloaded into the SAME engine (no new handle), in the order fp32, bf16, fp32 again, bf16 again, reload under bf16, fp32.  Two
trees compute the same when their outputs are equal line by line (tools/sampling_paths.py does the same for the sampling step, on UNET_TINY in fp32 only).

    python tools/engine_digests.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sampling_paths import digest  # noqa: E402

DEV = "cuda"


def unets():
    from oracle import golden_configs as G
    from tests.unet_cases import CASES
    for name, c in CASES.items():
        yield name, c["cfg"], c["B"], c["H"], c["W"], c["S_byt5"], c["n_img"], c["seed"]
    yield "UNET_TINY", G.UNET_TINY, 3, 16, 16, 3, 1, 301
    yield "UNET_VARIANT", G.UNET_VARIANT, 2, 8, 8, 3, 0, 302
    yield "UNET_MID", G.UNET_MID, 2, 16, 16, 5, 2, 303


def main():
    import torch

    import paella_amd
    from oracle import golden_configs as G
    from paella_amd import synth
    from tests.helpers import cond_for, to_dev, weights_for
    for name, cfg, B, H, W, S_byt5, n_img, seed in unets():
        m = paella_amd.Paella(**cfg)
        weights_for(m, sum(cfg["blocks"]))
        m = m.to(DEV).eval()
        g = torch.Generator().manual_seed(seed)
        x = torch.randint(0, cfg["num_labels"], (B, H, W), generator=g).to(DEV)
        r = torch.rand(B, generator=g).to(DEV)
        c = to_dev(cond_for(cfg, B, S_byt5, n_img, G.COND_SEED + seed), DEV)

        def logits(tag, mode):
            m.set_gemm_precision(mode)
            out = m.forward_prepared(x, r, m.prepare_cond(**c))
            torch.cuda.synchronize()
            print("unet  %-13s %-15s %s" % (name, tag, digest([out])), flush=True)

        logits("fp32", "fp32")
        handle = m._engine()
        logits("bf16", "bf16")
        logits("fp32 again", "fp32")
        logits("bf16 again", "bf16")
        with torch.no_grad():
            for i, p in enumerate(m.parameters()):
                p.mul_(1.0 + 0.03125 * (i % 3))
        logits("reload bf16", "bf16")
        logits("reload fp32", "fp32")
        assert m._engine() is handle, "the engine was recreated"
    for name, vc in (("VQ_TINY_F4", G.VQ_TINY_F4), ("VQ_TINY_F8", G.VQ_TINY_F8)):
        v = paella_amd.VQModel(**vc)
        synth.randomize_(v, seed=0)
        v = v.to(DEV).eval()
        g = torch.Generator().manual_seed(7)
        idx = torch.randint(0, vc["codebook_size"], (2, 4, 6), generator=g).to(DEV)
        img = torch.rand(2, 3, 4 << vc["levels"], 2 << vc["levels"], generator=g).to(DEV)
        for mode in ("fp32", "bf16", "fp32"):
            v.set_gemm_precision(mode)
            dec, enc = v.decode_indices(idx), v.encode(img)
            torch.cuda.synchronize()
            print("vqgan %-13s %-15s decode %s  encode %s" % (name, mode, digest([dec]), digest([t for t in enc if torch.is_tensor(t)])), flush=True)


if __name__ == "__main__":
    main()
