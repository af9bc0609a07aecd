"""Helpers over the golden fixtures that more than one test module uses (a plain module, not a conftest)."""


def sub(t, prefix):
    return {k[len(prefix):]: v for k, v in t.items() if k.startswith(prefix)}


def g15_case(golden):
    """Everything the G15 replay needs, rebuilt from the manifest: the DiT weights are G7's, the VAE decoder and the latent
    upsampler come from the oracle's seeded initialisers (fingerprints checked, so an RNG drift fails loudly here and not
    as a parity miss), the prompts go through the same fake T5 as in the generator."""
    from oracle import upsampler as ou, vae as ov
    from fake_t5 import FakeTextEncoder, FakeTokenizer
    t, meta = golden("g15_multiscale_call")
    w, _ = golden("g7_pipeline_call")
    sd = sub(w, "w.")
    vsd = ov.init_state_dict(meta["vae_cfg"], seed=meta["vae_seed"])
    usd = ou.init_state_dict(meta["upsampler_cfg"], seed=meta["upsampler_seed"])

    def fingerprint(d):
        return float(sum(v.double().abs().sum() for v in d.values()))

    assert abs(fingerprint(vsd) - meta["vae_fingerprint"]) < 1e-6 * meta["vae_fingerprint"], "seeded VAE weights drifted"
    assert abs(fingerprint(usd) - meta["upsampler_fingerprint"]) < 1e-6 * meta["upsampler_fingerprint"]
    tok, enc = FakeTokenizer(), FakeTextEncoder(meta["dit_cfg"]["caption_channels"], seed=meta["text_encoder_seed"]).eval()
    return t, meta, sd, vsd, usd, tok, enc
