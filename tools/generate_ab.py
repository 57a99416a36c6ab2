"""generate() against the loop it replaces, in one process: per-token time of
MambaTTSDecoder.generate (one hipGraph replay per token, sampler and counters
on the device) and of decode_step + torch softmax / top-k / cumsum /
multinomial with the token kept on the device, at C4 (12 layers, d_model
1024, B = 32, bf16) over 512 steps, timed with HIP events, three interleaved
repeats each; vocabulary 10 and 1024, greedy and top_k=50 / top_p=0.9.
--ragged runs the ragged-prompt leg instead (vocabulary 1024, greedy): a
(32, 512) right-padded prompt with lengths uniform in [64, 512] -- the
prefill with prompt_lengths against the rectangular prefill and against
stepping the prompt columns through decode_step, and the per-token time of
the ragged continuation against the rectangular one (the same graph).
--rows runs the per-row sampling leg instead (vocabulary 10 and 1024, top_k=50
/ top_p=0.9): (a) the scalar path, (b) the per-row path with the same
settings in every row and no penalty, (c) the per-row path with
repetition_penalty 1.3 over a window of 64.
--session runs the continuous-batching leg instead: (1) us per replay of a
DecodeSession's graph (32 slots, every slot live) against generate()'s
rows-path graph, same controls, vocabulary 10 and 1024, three interleaved
repeats; (2) 128 requests with caps uniform in [200, 1000] (fixed seed)
through generate_requests on 32 slots against static batches of 32 through
generate(): replays (derived from plan_slots beforehand, and made) and wall
time.
--long-keys runs the long-conditioning leg instead (--steps 256): us per token
of a session with every slot live at train.py's widths (8 layers, d_model 512,
max_keys 5248; 1, 8 and 32 slots) and at C4's (max_keys 1024, 32 slots), (p)
with the parent's routing (DecodeEngine.OPTIONS["split_keys"] off), (s) on the
split-key kernel with every request at max_keys, (r) on it with request key
counts uniform in [600, max_keys]; three interleaved repeats.
--logprobs runs the token log-probability leg instead (vocabulary 10 and 1024,
top_k=50 / top_p=0.9, penalty 1.3 over a window of 64 on the per-row paths):
generate() on the scalar path, generate() on the per-row path and a session's
run(n) with every slot live, each with the feature off and on, three
interleaved repeats in one process.  With AB_PKG naming another commit's
package directory (its mamba_decoder.py, mtts/ and libmtts.so) that package
is timed instead; one that does not know the feature runs the "off" cases
only, which are the same launches in both.
--shared-keys runs the parallel-samples leg instead (--steps 256): train.py's
widths (8 layers, d_model 512), max_keys 5248, 32 slots, every slot live and
every request at max_keys, as 32 x 1, 16 x 2, 8 x 4 and 4 x 8 (groups x
samples of one request, admit_samples): us per token of a share_keys session
(one copy of a group's K/V, loaded once per step for the group) against a
plain session whose members hold copies (what n unrelated requests cost), five
interleaved repeats in one process, median, min and max; then the wall time of
one admit_samples of 4 against four admits.
--kv-fp8 runs the FP8 K/V leg instead (--steps 256): the shapes of --long-keys
(train.py's widths at max_keys 5248 with 1, 8 and 32 slots, C4's at max_keys
1024 with 32 slots; every request at max_keys, and key counts uniform in
[600, max_keys]), us per token of a session with bf16 K/V against one opened
with kv_dtype="fp8", both on the split-key kernel, five interleaved repeats in
one process, median, min and max; the K/V bytes each session holds; then the
wall time of one admit and of one admit_samples of 4, both ways.
python tools/generate_ab.py [--steps 512] [--ragged | --rows | --session | --long-keys | --logprobs | --shared-keys |
                             --kv-fp8] [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "mamba-tts-project_amd"))
import torch  # noqa: E402

import bench  # noqa: E402

if os.environ.get("AB_PKG"):    # another commit's package, ahead of this tree's (bench.py has put that first)
    sys.path.insert(0, os.path.abspath(os.environ["AB_PKG"]))


def torch_draw(logits, temperature, top_k, top_p):
    """What a caller writes around decode_step today; returns (B, 1) int64."""
    if temperature == 0:
        return logits.argmax(-1, keepdim=True)
    x = logits.float() / temperature
    if top_k > 0:
        kth = torch.topk(x, min(top_k, x.shape[-1]), dim=-1).values[:, -1:]
        x = x.masked_fill(x < kth, float("-inf"))
    p, idx = torch.sort(torch.softmax(x, -1), dim=-1, descending=True)
    if top_p < 1:
        p = p.masked_fill(torch.cumsum(p, -1) - p >= top_p, 0.0)
    return idx.gather(1, torch.multinomial(p, 1))


def xpk(ses):
    """The session steps on packed activations (a package timed through AB_PKG may keep the flag on the engine)."""
    eng = ses.eng
    return eng.ctx.xpk if hasattr(eng.ctx, "xpk") else eng.xpk


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def ragged_leg(n, dev, lines):
    import mamba_decoder
    vocab, Tp = 1024, 512
    c = dict(bench.C2)
    c["B"] = 32
    torch.manual_seed(0)
    m = mamba_decoder.MambaTTSDecoder(vocab, d_model=c["d_model"], n_layers=c["n_layers"], n_heads=c["n_heads"],
                                      d_ff=c["d_ff"], d_style=c["d_style"]).to(dev).eval()
    m.compute_dtype = torch.bfloat16
    _, text, z, mask = bench.make_batch(c, dev, 7)
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(64, Tp + 1, (32,), generator=g)
    lens[0] = Tp
    prompt = torch.randint(0, vocab, (32, Tp), generator=g).to(dev)
    kw = dict(temperature=0.0, text_mask=mask, seed=1)

    def rect(k):
        m.generate(text, z, k, prompt_tokens=prompt, **kw)

    def rag(k):
        m.generate(text, z, k, prompt_tokens=prompt, prompt_lengths=lens, **kw)

    def steps():   # what a caller does without prompt_lengths: one decode_step per prompt column
        with torch.no_grad():
            states = [None] * c["n_layers"]
            for t in range(Tp):
                _, states = m.decode_step(prompt[:, t:t + 1], text, z, states, t, text_mask=mask)

    for f in (rect, rag):
        f(n + 1)
    steps()
    res = {k: [] for k in ("rect1", "rag1", "rectn", "ragn", "steps")}
    for _ in range(3):
        res["rect1"].append(timed(lambda: rect(1)))
        res["rag1"].append(timed(lambda: rag(1)))
        res["rectn"].append(timed(lambda: rect(n + 1)))
        res["ragn"].append(timed(lambda: rag(n + 1)))
        res["steps"].append(timed(steps))
    fmt = lambda v: f"{min(v):8.2f} (" + " ".join(f"{x:.2f}" for x in v) + ")"  # noqa: E731
    lines.append(f"ragged prompts, C4 (12L d=1024 B=32 bf16), vocab {vocab}, Tp {Tp}, lengths uniform in [64, {Tp}] "
                 f"(mean {lens.float().mean():.0f}); ms, three repeats, min first")
    lines.append(f"prefill + first token, rectangular (32 x {Tp})   {fmt(res['rect1'])}")
    lines.append(f"prefill + first token, prompt_lengths            {fmt(res['rag1'])}")
    lines.append(f"{Tp} decode_steps over the prompt columns          {fmt(res['steps'])}")
    per = {k: [(a - b) * 1e3 / n for a, b in zip(res[k + "n"], res[k + "1"])] for k in ("rect", "rag")}
    lines.append(f"us per token after the prefill ({n} tokens): rectangular " + fmt(per["rect"]).strip()
                 + "  ragged " + fmt(per["rag"]).strip() + f"  graphs captured {len(m._engine.gen_graphs)}")
    for ln in lines[-5:]:
        print(ln, flush=True)


def rows_leg(n, dev, lines):
    import mamba_decoder
    lines.append(f"per-row sampling, C4 (12L d=1024 B=32 bf16), {n} steps, top_k=50 top_p=0.9, us per token "
                 "(three interleaved repeats, min first; spread = max - min)")
    for vocab in (10, 1024):
        c = dict(bench.C2)
        c["B"] = 32
        torch.manual_seed(0)
        m = mamba_decoder.MambaTTSDecoder(vocab, d_model=c["d_model"], n_layers=c["n_layers"], n_heads=c["n_heads"],
                                          d_ff=c["d_ff"], d_style=c["d_style"]).to(dev).eval()
        m.compute_dtype = torch.bfloat16
        _, text, z, mask = bench.make_batch(c, dev, 7)
        kw = dict(top_k=50, top_p=0.9, text_mask=mask, seed=1)
        cases = (("(a) scalar path", dict(temperature=1.0)),
                 ("(b) per-row path, no penalty", dict(temperature=[1.0] * 32)),
                 ("(c) per-row path, penalty 1.3 window 64",
                  dict(temperature=[1.0] * 32, repetition_penalty=1.3, repetition_window=64)))
        for _, extra in cases:
            m.generate(text, z, n, **kw, **extra)      # capture / warm up
        res = [[] for _ in cases]
        for _ in range(3):
            for r, (_, extra) in zip(res, cases):
                r.append(timed(lambda: m.generate(text, z, n, **kw, **extra)) * 1e3 / n)
        for (name, _), r in zip(cases, res):
            lines.append(f"vocab {vocab:5d} {name:42s} {min(r):7.1f} (" + " ".join(f"{v:.1f}" for v in r)
                         + f")  spread {max(r) - min(r):.1f}  vs (a) {min(r) - min(res[0]):+.1f}")
            print(lines[-1], flush=True)
        lines.append(f"vocab {vocab:5d} graphs captured {len(m._engine.gen_graphs)}")


def session_leg(n, dev, lines):
    import time

    import mamba_decoder
    from mtts.session import plan_slots
    B = 32
    lines.append(f"decode session vs generate() rows path, C4 (12L d=1024 B=32 bf16), {n} steps, top_k=50 top_p=0.9, "
                 "us per token (three interleaved repeats, min first; spread = max - min).  generate() is timed as a "
                 "call (its per-call host work and final synchronisation spread over the steps), the session as "
                 "run(n) alone with every slot live")
    caps = torch.randint(200, 1001, (128,), generator=torch.Generator().manual_seed(11)).tolist()
    static = sum(max(caps[i:i + B]) for i in range(0, len(caps), B))
    _, planned = plan_slots(caps, B, 16)
    for vocab in (10, 1024):
        c = dict(bench.C2)
        c["B"] = B
        torch.manual_seed(0)
        m = mamba_decoder.MambaTTSDecoder(vocab, d_model=c["d_model"], n_layers=c["n_layers"], n_heads=c["n_heads"],
                                          d_ff=c["d_ff"], d_style=c["d_style"]).to(dev).eval()
        m.compute_dtype = torch.bfloat16
        _, text, z, mask = bench.make_batch(c, dev, 7)
        kw = dict(top_k=50, top_p=0.9, text_mask=mask, seed=list(range(1, B + 1)), temperature=[1.0] * B)
        ses = m.open_session(B, text.shape[1], repetition_window=64)

        def gen(penalty):
            m.generate(text, z, n, repetition_penalty=penalty, repetition_window=64, **kw)

        def fill(penalty):
            for r in range(B):
                ses.admit(r, text[r], z[r], text_mask=mask[r], max_new_tokens=n, temperature=1.0, top_k=50,
                          top_p=0.9, seed=r + 1, repetition_penalty=penalty)

        def drain():
            for r in ses.poll():
                ses.take(r)

        def session(penalty):
            fill(penalty)
            t = timed(lambda: ses.run(n))
            drain()
            return t

        cases = (("(b) generate, per-row path, no penalty", lambda: timed(lambda: gen(None))),
                 ("(s) session, no penalty", lambda: session(None)),
                 ("(c) generate, per-row path, penalty 1.3 window 64", lambda: timed(lambda: gen(1.3))),
                 ("(t) session, penalty 1.3 window 64", lambda: session(1.3)))
        for _, f in cases:
            f()                                            # capture / warm up
        res = [[] for _ in cases]
        for _ in range(3):
            for r, (_, f) in zip(res, cases):
                r.append(f() * 1e3 / n)
        for i, ((name, _), r) in enumerate(zip(cases, res)):
            against = "" if i % 2 == 0 else f"  session - generate {min(r) - min(res[i - 1]):+.1f}"
            lines.append(f"vocab {vocab:5d} {name:50s} {min(r):7.1f} (" + " ".join(f"{v:.1f}" for v in r)
                         + f")  spread {max(r) - min(r):.1f}" + against)
            print(lines[-1], flush=True)
        lines.append(f"vocab {vocab:5d} graphs captured: generate {len(m._engine.gen_graphs)}, session {ses.captures}")
        # throughput: 128 requests, caps uniform in [200, 1000]
        reqs = [dict(text_hidden=text[i % B], z_style=z[i % B], text_mask=mask[i % B], max_new_tokens=caps[i],
                     temperature=1.0, top_k=50, top_p=0.9, seed=i + 1) for i in range(len(caps))]

        def static_batches():
            made = 0
            for i in range(0, len(caps), B):
                toks, _ = m.generate(text, z, caps[i:i + B], top_k=50, top_p=0.9, text_mask=mask,
                                     temperature=[1.0] * B, seed=list(range(i + 1, i + B + 1)))
                made += toks.shape[1]
            return made

        def wall(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            return out, time.perf_counter() - t0

        static_batches()                                   # warm up both
        m.generate_requests(reqs[:B], slots=B, max_keys=text.shape[1], check_every=16)
        made_s, t_s = wall(static_batches)
        (toks, _, made_c), t_c = wall(lambda: m.generate_requests(reqs, slots=B, max_keys=text.shape[1],
                                                                  check_every=16))
        assert [int(t.numel()) for t in toks] == caps
        lines.append(f"vocab {vocab:5d} 128 requests, caps uniform in [200, 1000] (sum {sum(caps)}): static batches of "
                     f"{B}: {made_s} replays (derived {static}), {t_s:.3f} s; session of {B} slots, check_every 16: "
                     f"{made_c} replays (derived {planned}), {t_c:.3f} s (session open and capture included); "
                     f"replay ratio {made_c / made_s:.3f} (derived {planned / static:.3f}), wall ratio {t_c / t_s:.3f}")
        print(lines[-1], flush=True)


def long_keys_leg(n, dev, lines):
    """Decode at the conditioning lengths the model has: a session with every
    slot live, us per token, (p) the parent's routing (OPTIONS["split_keys"]
    off: the unpacked step and the serial single-query kernel), (s) the
    split-key kernel with every request at max_keys, (r) the split-key kernel
    with request key counts uniform in [600, max_keys] (fixed seed)."""
    import mamba_decoder
    from mtts.decode import DecodeEngine
    vocab = 1024
    lines.append(f"decode over long conditioning, bf16, vocab {vocab}, {n} steps, top_k=50 top_p=0.9, every slot live, "
                 "us per token (three interleaved repeats in one process, min first; spread = max - min).  (p) parent "
                 "routing (split_keys off), (s) split-key kernel, every request at max_keys, (r) split-key kernel, "
                 "key counts uniform in [600, max_keys] (seed 5)")
    shapes = (("train.py widths (8L d=512 8 heads)", dict(n_layers=8, d_model=512, n_heads=8), 5248, (1, 8, 32)),
              ("C4 widths (12L d=1024 8 heads)", dict(n_layers=12, d_model=1024, n_heads=8), 1024, (32,)))
    for name, width, max_keys, slot_counts in shapes:
        torch.manual_seed(0)
        m = mamba_decoder.MambaTTSDecoder(vocab, d_ff=2048, d_style=256, **width).to(dev).eval()
        m.compute_dtype = torch.bfloat16
        d = width["d_model"]
        for slots in slot_counts:
            g = torch.Generator().manual_seed(5)
            text = torch.randn(slots, max_keys, d, generator=g).to(dev)
            z = torch.randn(slots, 256, generator=g).to(dev)
            counts = torch.randint(600, max_keys + 1, (slots,), generator=g).tolist()
            ses = {}
            for leg, on in (("p", False), ("s", True), ("r", True)):   # the routing is fixed at capture
                DecodeEngine.OPTIONS["split_keys"] = on
                try:
                    ses[leg] = m.open_session(slots, max_keys, repetition_window=64)
                finally:
                    DecodeEngine.OPTIONS["split_keys"] = True
            assert xpk(ses["s"]) and xpk(ses["r"]) and not xpk(ses["p"])

            def run(leg):
                s = ses[leg]
                for r in range(slots):
                    keys = counts[r] if leg == "r" else max_keys
                    s.admit(r, text[r, :keys], z[r], max_new_tokens=n, temperature=1.0, top_k=50, top_p=0.9,
                            seed=r + 1)
                t = timed(lambda: s.run(n))
                for r in s.poll():
                    s.take(r)
                return t * 1e3 / n

            for leg in ses:
                run(leg)                                       # warm up
            res = {leg: [] for leg in ses}
            for _ in range(3):
                for leg in ses:
                    res[leg].append(run(leg))
            mean = sum(counts) / slots
            for leg, what in (("p", "(p) parent routing"), ("s", "(s) split, all at max_keys"),
                              ("r", f"(r) split, key counts mean {mean:.0f}")):
                v = res[leg]
                against = "" if leg == "p" else f"  vs (p) {min(v) - min(res['p']):+.1f}"
                lines.append(f"{name}, max_keys {max_keys}, {slots:2d} slots  {what:36s} {min(v):8.1f} ("
                             + " ".join(f"{x:.1f}" for x in v) + f")  spread {max(v) - min(v):.1f}" + against)
                print(lines[-1], flush=True)
            del ses
            torch.cuda.empty_cache()


def kv_fp8_leg(n, dev, lines):
    """bf16 K/V against kv_dtype="fp8" at the shapes of long_keys_leg, both on
    the split-key kernel: us per token, the K/V bytes held, the admission."""
    import statistics
    import time

    import mamba_decoder
    vocab, reps = 1024, 5
    lines.append(f"FP8 conditioning K/V, bf16 step, vocab {vocab}, {n} steps, top_k=50 top_p=0.9, every slot live, us per "
                 f"token ({reps} interleaved repeats in one process: median [min max]; spread = max - min).  (b) bf16 "
                 "K/V, (f) kv_dtype='fp8', both on the split-key kernel; 'max': every request at max_keys, 'r': key "
                 "counts uniform in [600, max_keys] (seed 5).  K/V held: bytes of every layer's K/V tensors in the "
                 "session (bf16: k, v and the head-major copies; fp8: bytes and scales)")
    shapes = (("train.py widths (8L d=512 8 heads)", dict(n_layers=8, d_model=512, n_heads=8), 5248, (1, 8, 32)),
              ("C4 widths (12L d=1024 8 heads)", dict(n_layers=12, d_model=1024, n_heads=8), 1024, (32,)))

    def fmt(v):
        return f"{statistics.median(v):8.1f} [{min(v):.1f} {max(v):.1f}]  spread {max(v) - min(v):.1f}"

    for name, width, max_keys, slot_counts in shapes:
        torch.manual_seed(0)
        m = mamba_decoder.MambaTTSDecoder(vocab, d_ff=2048, d_style=256, **width).to(dev).eval()
        m.compute_dtype = torch.bfloat16
        d = width["d_model"]
        for slots in slot_counts:
            g = torch.Generator().manual_seed(5)
            text = torch.randn(slots, max_keys, d, generator=g).to(dev)
            z = torch.randn(slots, 256, generator=g).to(dev)
            counts = torch.randint(600, max_keys + 1, (slots,), generator=g).tolist()
            ses = {"b": m.open_session(slots, max_keys, repetition_window=64),
                   "f": m.open_session(slots, max_keys, repetition_window=64, kv_dtype="fp8")}
            assert xpk(ses["b"]) and xpk(ses["f"])
            held = {leg: s.cond.kv_bytes() for leg, s in ses.items()}
            kw = dict(temperature=1.0, top_k=50, top_p=0.9)

            def run(leg, ragged):
                s = ses[leg]
                for r in range(slots):
                    keys = counts[r] if ragged else max_keys
                    s.admit(r, text[r, :keys], z[r], max_new_tokens=n, seed=r + 1, **kw)
                t = timed(lambda: s.run(n))
                for r in s.poll():
                    s.take(r)
                return t * 1e3 / n

            cases = [(leg, ragged) for ragged in (False, True) for leg in ("b", "f")]
            for c in cases:
                run(*c)                                        # warm up
            res = {c: [] for c in cases}
            for _ in range(reps):
                for c in cases:
                    res[c].append(run(*c))
            mean = sum(counts) / slots
            for ragged, what in ((False, "max"), (True, f"r (mean {mean:.0f} keys)")):
                b, f = res[("b", ragged)], res[("f", ragged)]
                lines.append(f"{name}, max_keys {max_keys}, {slots:2d} slots, {what:20s} (b) {fmt(b)}   (f) {fmt(f)}   "
                             f"(f) - (b) {statistics.median(f) - statistics.median(b):+.1f}")
                print(lines[-1], flush=True)
            lines.append(f"{name}, max_keys {max_keys}, {slots:2d} slots, K/V held: (b) {held['b'] / 2**20:.1f} MiB   "
                         f"(f) {held['f'] / 2**20:.1f} MiB")
            print(lines[-1], flush=True)
            if slots >= 4 and slots == max(slot_counts):

                def admission(leg, together):
                    s = ses[leg]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if together:
                        s.admit_samples([0, 1, 2, 3], text[0], z[0], max_new_tokens=2, seed=1, **kw)
                    else:
                        s.admit(0, text[0], z[0], max_new_tokens=2, seed=1, **kw)
                    torch.cuda.synchronize()
                    t = (time.perf_counter() - t0) * 1e3
                    s.run(2)
                    for r in s.poll():
                        s.take(r)
                    return t

                acases = [(leg, tog) for tog in (False, True) for leg in ("b", "f")]
                for c in acases:
                    admission(*c)
                ares = {c: [] for c in acases}
                for _ in range(reps):
                    for c in acases:
                        ares[c].append(admission(*c))
                for tog, what in ((False, "one admit"), (True, "admit_samples of 4")):
                    lines.append(f"{name}, max_keys {max_keys}, {slots:2d} slots, {what}, wall ms with a synchronize on "
                                 "both sides: " + "   ".join(
                                     f"({leg}) {statistics.median(ares[(leg, tog)]):.2f} [{min(ares[(leg, tog)]):.2f} "
                                     f"{max(ares[(leg, tog)]):.2f}]" for leg in ("b", "f")))
                    print(lines[-1], flush=True)
            lines.append("graphs captured: " + " ".join(str(s.captures) for s in ses.values()))
            del ses
            torch.cuda.empty_cache()


def shared_keys_leg(n, dev, lines):
    """n samples of one request: a share_keys session against a plain one
    whose members hold copies of the K/V, then the admission itself."""
    import statistics
    import time

    import mamba_decoder
    vocab, slots, max_keys, d, reps = 1024, 32, 5248, 512, 5
    lines.append(f"parallel samples of one request, train.py widths (8L d=512 8 heads), bf16, vocab {vocab}, max_keys "
                 f"{max_keys}, {slots} slots, every slot live, every request at max_keys, {n} steps, top_k=50 top_p=0.9, "
                 f"us per token ({reps} interleaved repeats in one process: median [min max]; spread = max - min).  "
                 "(c) plain session, every member holds a copy of the K/V; (s) share_keys session, one copy per group")
    torch.manual_seed(0)
    m = mamba_decoder.MambaTTSDecoder(vocab, d_ff=2048, d_style=256, n_layers=8, d_model=d, n_heads=8).to(dev).eval()
    m.compute_dtype = torch.bfloat16
    g = torch.Generator().manual_seed(5)
    text = torch.randn(slots, max_keys, d, generator=g).to(dev)
    z = torch.randn(slots, 256, generator=g).to(dev)
    ses = {"c": m.open_session(slots, max_keys, repetition_window=64),
           "s": m.open_session(slots, max_keys, repetition_window=64, share_keys=True)}
    kw = dict(temperature=1.0, top_k=50, top_p=0.9)

    def fmt(v):
        return f"{statistics.median(v):8.1f} [{min(v):.1f} {max(v):.1f}]  spread {max(v) - min(v):.1f}"

    def run(leg, per):
        s = ses[leg]
        for i in range(slots // per):
            s.admit_samples(list(range(i * per, (i + 1) * per)), text[i], z[i], max_new_tokens=n, seed=i + 1, **kw)
        t = timed(lambda: s.run(n))
        for r in s.poll():
            s.take(r)
        assert s.state == ["idle"] * slots
        return t * 1e3 / n

    for per in (1, 2, 4, 8):
        for leg in ses:
            run(leg, per)                                      # warm up
        res = {leg: [] for leg in ses}
        for _ in range(reps):
            for leg in ses:
                res[leg].append(run(leg, per))
        diff = statistics.median(res["s"]) - statistics.median(res["c"])
        lines.append(f"{slots // per:2d} x {per}  (c) copies {fmt(res['c'])}   (s) shared {fmt(res['s'])}   "
                     f"(s) - (c) {diff:+.1f}")
        print(lines[-1], flush=True)

    lines.append("admission of 4 samples of one request, wall ms with a synchronize on both sides "
                 f"({reps} interleaved repeats: median [min max]): four admit()s, admit_samples of 4 into a plain "
                 "session (copies), admit_samples of 4 into a share_keys session")
    for prompt in (0, 64):
        pt = torch.randint(0, vocab, (prompt,), generator=g).to(dev) if prompt else None

        def admission(leg, together):
            s = ses[leg]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if together:
                s.admit_samples([0, 1, 2, 3], text[0], z[0], max_new_tokens=2, seed=1, prompt_tokens=pt, **kw)
            else:
                for r in range(4):
                    s.admit(r, text[0], z[0], max_new_tokens=2, seed=r + 1, prompt_tokens=pt, **kw)
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) * 1e3
            s.run(2)
            for r in s.poll():
                s.take(r)
            return t

        cases = (("four admits", "c", False), ("admit_samples, copies", "c", True), ("admit_samples, shared", "s", True))
        for _, leg, tog in cases:
            admission(leg, tog)
        res = [[] for _ in cases]
        for _ in range(reps):
            for r, (_, leg, tog) in zip(res, cases):
                r.append(admission(leg, tog))
        lines.append(f"prompt of {prompt:2d} tokens: " + "   ".join(
            f"{name} {statistics.median(r):.2f} [{min(r):.2f} {max(r):.2f}]" for (name, _, _), r in zip(cases, res)))
        print(lines[-1], flush=True)
    lines.append("graphs captured: " + " ".join(str(s.captures) for s in ses.values()))
    print(lines[-1], flush=True)


def logprobs_leg(n, dev, lines):
    import inspect

    import mamba_decoder
    B = 32
    has = "return_logprobs" in inspect.signature(mamba_decoder.MambaTTSDecoder.generate).parameters
    lines.append(f"token log-probabilities, C4 (12L d=1024 B=32 bf16), {n} steps, top_k=50 top_p=0.9, us per token "
                 "(three interleaved repeats in one process, min first; spread = max - min); package "
                 + os.path.relpath(os.path.dirname(mamba_decoder.__file__), os.path.join(os.path.dirname(__file__), ".."))
                 + ("" if has else " (no log-probabilities: off cases only)"))
    for vocab in (10, 1024):
        c = dict(bench.C2)
        c["B"] = B
        torch.manual_seed(0)
        m = mamba_decoder.MambaTTSDecoder(vocab, d_model=c["d_model"], n_layers=c["n_layers"], n_heads=c["n_heads"],
                                          d_ff=c["d_ff"], d_style=c["d_style"]).to(dev).eval()
        m.compute_dtype = torch.bfloat16
        _, text, z, mask = bench.make_batch(c, dev, 7)
        kw = dict(top_k=50, top_p=0.9, text_mask=mask, seed=1)
        rows = dict(temperature=[1.0] * B, repetition_penalty=1.3, repetition_window=64)
        sessions = {False: m.open_session(B, text.shape[1], repetition_window=64)}
        if has:
            sessions[True] = m.open_session(B, text.shape[1], repetition_window=64, logprobs=True)

        def gen(extra, on):
            flag = dict(return_logprobs=True) if on else {}
            return timed(lambda: m.generate(text, z, n, **kw, **extra, **flag))

        def session(on):
            ses = sessions[on]
            for r in range(B):
                ses.admit(r, text[r], z[r], text_mask=mask[r], max_new_tokens=n, temperature=1.0, top_k=50,
                          top_p=0.9, seed=r + 1, repetition_penalty=1.3)
            t = timed(lambda: ses.run(n))
            for r in ses.poll():
                ses.take(r)
            return t

        cases = [("generate, scalar path", lambda on: gen(dict(temperature=1.0), on)),
                 ("generate, per-row path, penalty 1.3", lambda on: gen(rows, on)),
                 ("session, penalty 1.3", session)]
        cases = [(name + (", logprobs" if on else ""), f, on) for name, f in cases for on in ((False, True) if has
                                                                                            else (False,))]
        for _, f, on in cases:
            f(on)                                          # capture / warm up
        res = [[] for _ in cases]
        for _ in range(3):
            for r, (_, f, on) in zip(res, cases):
                r.append(f(on) * 1e3 / n)
        for i, ((name, _, on), r) in enumerate(zip(cases, res)):
            against = f"  on - off {min(r) - min(res[i - 1]):+.1f}" if on else ""
            lines.append(f"vocab {vocab:5d} {name:46s} {min(r):7.1f} (" + " ".join(f"{v:.1f}" for v in r)
                         + f")  spread {max(r) - min(r):.1f}" + against)
            print(lines[-1], flush=True)
        lines.append(f"vocab {vocab:5d} graphs captured: generate {len(m._engine.gen_graphs)}, sessions "
                     + " ".join(str(s.captures) for s in sessions.values()))
        print(lines[-1], flush=True)
        del sessions
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--ragged", action="store_true", help="run the ragged-prompt leg instead")
    ap.add_argument("--rows", action="store_true", help="run the per-row sampling leg instead")
    ap.add_argument("--session", action="store_true", help="run the continuous-batching leg instead")
    ap.add_argument("--long-keys", action="store_true", help="run the long-conditioning decode leg instead "
                    "(profiles/decode_long_keys.txt: --steps 256)")
    ap.add_argument("--logprobs", action="store_true", help="run the token log-probability leg instead "
                    "(profiles/sample_logprobs_ab.txt)")
    ap.add_argument("--shared-keys", action="store_true", help="run the parallel-samples leg instead "
                    "(profiles/shared_keys_ab.txt: --steps 256)")
    ap.add_argument("--kv-fp8", action="store_true", help="run the FP8 K/V leg instead "
                    "(profiles/kv_fp8_ab.txt: --steps 256)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import mamba_decoder
    dev = "cuda"
    n = args.steps
    if args.ragged or args.rows or args.session or args.long_keys or args.logprobs or args.shared_keys or args.kv_fp8:
        lines = []
        (kv_fp8_leg if args.kv_fp8 else ragged_leg if args.ragged else rows_leg if args.rows else session_leg if args.session
         else long_keys_leg if args.long_keys else shared_keys_leg if args.shared_keys else logprobs_leg)(n, dev, lines)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    lines = [f"generate vs decode_step + torch sampling, C4 (12L d=1024 B=32 bf16), {n} steps, us per token "
             "(three repeats; spread = max - min of the loop's)"]
    for vocab in (10, 1024):
        c = dict(bench.C2)
        c["B"] = 32
        torch.manual_seed(0)
        m = mamba_decoder.MambaTTSDecoder(vocab, d_model=c["d_model"], n_layers=c["n_layers"], n_heads=c["n_heads"],
                                          d_ff=c["d_ff"], d_style=c["d_style"]).to(dev).eval()
        m.compute_dtype = torch.bfloat16
        _, text, z, mask = bench.make_batch(c, dev, 7)
        for name, kw in (("greedy", dict(temperature=0.0)),
                         ("top_k=50 top_p=0.9", dict(temperature=1.0, top_k=50, top_p=0.9))):
            def gen():
                m.generate(text, z, n, text_mask=mask, seed=1, **kw)

            def loop():
                with torch.no_grad():
                    tok = torch.zeros(32, 1, dtype=torch.long, device=dev)
                    states = [None] * c["n_layers"]
                    for t in range(n):
                        lg, states = m.decode_step(tok, text, z, states, t, text_mask=mask)
                        tok = torch_draw(lg[:, 0], kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0))

            gen()     # capture / warm up both paths
            loop()
            tg, tl = [], []
            for _ in range(3):
                tg.append(timed(gen) * 1e3 / n)
                tl.append(timed(loop) * 1e3 / n)
            lines.append(f"vocab {vocab:5d} {name:20s} generate {min(tg):7.1f} (" + " ".join(f"{v:.1f}" for v in tg)
                         + f")  loop {min(tl):7.1f} (" + " ".join(f"{v:.1f}" for v in tl)
                         + f")  loop spread {max(tl) - min(tl):.1f}  generate - loop {min(tg) - min(tl):+.1f}")
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
