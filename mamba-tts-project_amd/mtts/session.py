"""Continuous batching for MambaTTSDecoder: a decode session whose rows
("slots") hold requests admitted at different times.

generate() is a batch call: every row starts together and a row that has
reached its cap idles until the longest one is done.  A Mamba decoder keeps
O(1) state per row, so a finished row can be handed to the next request at
once.  DecodeSession keeps everything a request owns as one row of static
device buffers -- its conditioning K/V over `max_keys` keys, key-padding mask,
key count (all the split-key attention reads of a long key side) and FiLM rows
in the context's Conditioning (mtts/conditioning.py, whose row operations it
uses); conv / SSM states, token, position, sampler controls, history -- and replays
ONE captured graph of the engine's decode step plus the slot form of the
sampler (ops.sample_tokens_slots: the history column is the row's own
draw count, finished rows keep their tokens and their position).  Admitting a
request rewrites its slot's rows in place, stream-ordered; no admission,
control value or seed captures again.  A request's random stream is a function
of (seed, tokens drawn so far, v) and every kernel of the step is row-wise, so
its tokens do not depend on its slot, its neighbours or the schedule.

admit_samples() puts n samples of one request into n slots for one K/V
projection and one prefill; in a session opened with share_keys the group also
keeps ONE copy of its K/V, in the rows of its first slot, which every member
reads through the session's (slots,) kv_rows buffer (the split-key attention
loads it once per step for the whole group, bit-identically), and that slot
stays reserved ("lent") until every member has been taken.

A session opened with kv_dtype="fp8" keeps the conditioning K/V as OCP FP8
bytes with one fp32 scale per (slot, head) -- (slots, H, max_keys, hd) uint8
per layer and operand, a quarter of the four bf16 images a packed session
holds -- allocated as such and quantised into per admission (Conditioning.idle
/ write), and the captured step reads them through the fp8 form of the
split-key attention (DecodeEngine.generate's kv_dtype has the definition).

plan_slots() is the refill policy as a pure host function;
generate_requests() runs a queue of requests through a session by it.
"""
from __future__ import annotations

import torch

from . import ops
from .conditioning import Conditioning
from .context import DecodeContext
from .decode import (DecodeEngine, _check_request, _check_vocab_ids, _check_window, _is_scalar, capture_graph,
                     check_kv_dtype, check_split_keys, sampler_buffers)


def plan_slots(caps, slots, check_every, prefilled=None, samples=None):
    """The refill policy of generate_requests for length caps `caps` (one per
    request, in order) on `slots` rows: admit in order into the lowest free
    slot; replay min(check_every, the largest number of tokens a live row has
    left) times; take what has finished; refill.  prefilled[i] true: request
    i draws its first token at admission (a prompt of more than one token),
    so it needs one replay less.  samples[i] = n: request i is n samples of
    one request (admit_samples); it is admitted once n slots are free, into
    the n lowest, and until then blocks the requests behind it; its answer is
    its list of slots (samples[i] None: one slot, an integer, as without
    `samples`).  Returns (slot of every request, replays)."""
    caps = [int(c) for c in caps]
    slots, check_every = int(slots), int(check_every)
    if slots < 1 or check_every < 1 or any(c < 1 for c in caps):
        raise ValueError("plan_slots: slots, check_every and every cap must be >= 1")
    pre = [False] * len(caps) if prefilled is None else [bool(p) for p in prefilled]
    if len(pre) != len(caps):
        raise ValueError("plan_slots: prefilled must hold one value per request")
    want = [None] * len(caps) if samples is None else [None if n is None else int(n) for n in samples]
    if len(want) != len(caps):
        raise ValueError("plan_slots: samples must hold one value per request")
    if any(n is not None and not 1 <= n <= slots for n in want):
        raise ValueError(f"plan_slots: every samples value must be in [1, slots = {slots}]")
    left = [None] * slots                   # tokens the slot's request has still to draw (None: free)
    where, nxt, replays = [], 0, 0
    while nxt < len(caps) or any(v is not None for v in left):
        while nxt < len(caps):
            free = [s for s in range(slots) if left[s] is None]
            n = 1 if want[nxt] is None else want[nxt]
            if len(free) < n:               # waits for slots, and so does every request behind it
                break
            for s in free[:n]:
                left[s] = caps[nxt] - (1 if pre[nxt] else 0)
            where.append(free[0] if want[nxt] is None else free[:n])
            nxt += 1
        n = min(check_every, max(v for v in left if v is not None))
        replays += n
        left = [None if v is None or v - n <= 0 else v - n for v in left]
    return where, replays


class DecodeSession:
    """See the module docstring; made by MambaTTSDecoder.open_session."""

    CAPTURES = 0        # graphs captured by every session of the process (tests count them)

    @torch.no_grad()
    def __init__(self, model, slots, max_keys, *, eos_id=None, pad_id=0, repetition_window=64, use_graph=True,
                 logprobs=False, share_keys=False, kv_dtype=None):
        m = self.m = model
        V = m.head.weight.shape[0]
        slots, max_keys = int(slots), int(max_keys)
        if slots < 1 or max_keys < 1:
            raise ValueError("open_session: slots and max_keys must be >= 1")
        _check_vocab_ids("open_session", V, pad_id, eos_id)
        _check_window("open_session", repetition_window)
        dev = m.token_embed.weight.device
        if dev.type != "cuda":
            raise RuntimeError("open_session runs on the HIP kernels only (no CPU path)")
        self.slots, self.max_keys, self.V = slots, max_keys, V
        self.eos, self.pad, self.window = None if eos_id is None else int(eos_id), int(pad_id), repetition_window
        # FP8 keys: the split-key attention's fp8 form reads them; checked before anything is allocated
        check_kv_dtype("open_session", m, kv_dtype, max_keys)
        if kv_dtype is not None and share_keys:
            raise ValueError("open_session: kv_dtype='fp8' with share_keys is not built (the shared-key kernel "
                             "measured no gain and has no fp8 form)")
        self.kv_dtype = kv_dtype
        self.use_graph = bool(use_graph)
        self.logprobs = bool(logprobs)                      # decided here: it selects the one capture
        self.share_keys = bool(share_keys)                  # so is this: the captured step reads K/V through kv_rows
        if self.share_keys:                                 # only the split-key kernel takes a K/V row per query row
            check_split_keys("open_session", "share_keys", m, max_keys, f"max_keys = {max_keys}")
        self.dev = dev
        cd = self.cd = m._cd()
        P = self.P = m.pos_embed.num_embeddings
        # a private engine over a context of `slots` idle rows, built and routed as generate()'s is
        eng = self.eng = DecodeEngine(m, use_graph=False)
        cond = self.cond = Conditioning.idle(slots, max_keys, cd, dev, kv_dtype, eng.OPTIONS["split_keys"], share_keys)
        self.kpm, self.kv_lens, self.kv_rows = cond.kpm, cond.kv_lens, cond.kv_rows
        eng.adopt(DecodeContext.build(m, cond, slots, eng.use_rows), slots, dev)
        eng.tok_buf.fill_(self.pad)
        # the batch-1 prefill runs on an engine of its own states; the context, constants and routing, is shared
        self.pre = DecodeEngine(m, use_graph=False)
        self.pre.adopt(eng.ctx, 1, dev)
        # length (int64) and finished (int32) share one allocation: a poll is one copy
        self._raw = torch.zeros(12 * slots, dtype=torch.uint8, device=dev)
        self._raw_host = torch.zeros(12 * slots, dtype=torch.uint8, pin_memory=True)
        self.length = self._raw[:8 * slots].view(torch.int64)
        self.finished = self._raw[8 * slots:].view(torch.int32)
        self.finished.fill_(1)
        self.g = sampler_buffers(slots, V, P, dev, logprobs=self.logprobs)
        self.logits = torch.zeros(slots, V, device=dev, dtype=cd)
        # idle -> live (admit) -> done (poll) -> idle (take); a slot whose K/V rows other slots still read goes
        # done -> lent (take) -> idle (the last of them taken)
        self.state = ["idle"] * slots
        self.holder = list(range(slots))                    # the slot whose K/V rows the slot reads
        self.borrowers = [set() for _ in range(slots)]      # the other slots that read this slot's K/V rows
        self.lengths = [0] * slots
        self.graph = None
        self.captures = 0
        self.replays = 0
        if self.use_graph:                                  # once, with every slot idle
            self.graph, self.logits = capture_graph(self._body, self._idle_all)
            self.captures += 1
            DecodeSession.CAPTURES += 1

    # -- the step ---------------------------------------------------------------
    def _sample(self, logits, rows):
        """The slot form of the sampler on `rows` (a slice) of the slot buffers."""
        g, eng = self.g, self.eng
        ops.sample_tokens_slots(
            logits, temperature=g["temperature"][rows], top_k=g["top_k"][rows], top_p=g["top_p"][rows],
            seed=g["row_seed"][rows], draw=g["draw"][rows], penalty=g["penalty"][rows], window=self.window,
            max_length=g["max_length"][rows], logit_bias=g["bias"][rows], advance=True, out=eng.tok_buf[rows],
            history=g["hist"][rows], eos_id=self.eos, pad_id=self.pad, finished=self.finished[rows],
            length=self.length[rows], unfinished=g["unfinished"] if rows == slice(None) else None,
            pos=eng.step_pos[rows] if eng.ctx.fused else None,
            logprob_history=g["lp_hist"][rows] if self.logprobs else None)
        if not eng.ctx.fused:                               # the generic step's int64 positions: the same rule
            eng.step_pos[rows] += (self.finished[rows] == 0).to(torch.int64)

    def _body(self):
        """Step + sampler.  Under a graph the step's own output is the static
        logits buffer (returned: the capture keeps it); launched directly, the
        output is copied into self.logits."""
        eng = self.eng
        lg = eng.step_fn(self.logprobs)(eng.tok_buf, eng.pos_buf, eng.states)[:, 0]
        if not self.use_graph:
            self.logits.copy_(lg)
            lg = self.logits
        self._sample(lg, slice(None))
        return lg

    def _idle_all(self):
        eng = self.eng
        for cs, ss in eng.states:
            cs.zero_()
            ss.zero_()
        eng.tok_buf.fill_(self.pad)
        eng.set_pos(0)
        self.finished.fill_(1)
        self.length.zero_()
        self.g["draw"].zero_()

    @torch.no_grad()
    def run(self, n=1):
        """n tokens for every live slot: n replays of the captured graph (or n
        direct launches of the same body under decode_mode "eager")."""
        step = self.graph.replay if self.graph is not None else self._body
        for _ in range(int(n)):
            step()
        self.replays += int(n)

    # -- requests ---------------------------------------------------------------
    def _check_slot(self, slot):
        if isinstance(slot, bool) or not isinstance(slot, int) or not 0 <= slot < self.slots:
            raise ValueError(f"session: slot must be an integer in [0, {self.slots})")

    @torch.no_grad()
    def admit(self, slot, text_hidden, z_style, *, max_new_tokens, text_mask=None, ref_hidden=None, ref_mask=None,
              prompt_tokens=None, start_token=0, temperature=1.0, top_k=0, top_p=1.0, seed=0,
              repetition_penalty=None, logit_bias=None):
        """Put one request into an idle slot: unbatched tensors, or tensors
        with a leading 1.  The arguments mean what they mean in generate();
        `seed` is the request's own stream seed (no row_seeds expansion).
        Every check comes first; then the slot's rows are rewritten in place,
        stream-ordered.  The conditioning [ref ‖ text] is padded to max_keys
        keys before its K/V projection, so every admission runs the same GEMM
        shape and a request's K/V does not depend on when or where it was
        admitted.  A prompt of more than one token is prefilled at batch 1
        through the scan path and the first token drawn here."""
        self._check_slot(slot)
        self._admit("admit", [slot], seed, False, text_hidden, z_style, max_new_tokens, text_mask, ref_hidden, ref_mask,
                    prompt_tokens, start_token, temperature, top_k, top_p, repetition_penalty, logit_bias)

    @torch.no_grad()
    def admit_samples(self, slots, text_hidden, z_style, *, max_new_tokens, text_mask=None, ref_hidden=None,
                      ref_mask=None, prompt_tokens=None, start_token=0, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                      repetition_penalty=None, logit_bias=None):
        """n = len(slots) samples of ONE request into n distinct idle slots;
        the other arguments are admit's.  Every check comes first.  The
        padded K/V projection of every layer, the FiLM rows and (a prompt of
        more than one token) the prefill are computed once; member j gets the
        seed ops.row_seeds(seed, n)[j], its own controls and history, a copy
        of the prefilled states, and draws its own first token from the
        shared prefill logits.  Its tokens and log-probabilities are those of
        admit(slot, ..., seed=row_seeds(seed, n)[j]) alone in any session.
        In a share_keys session the K/V, mask row and key count are written
        into slots[0]'s rows only and every member's kv_rows entry names that
        slot: one load of the keys per step serves the group.  slots[0] then
        stays reserved until every member has been taken (take()).  In any
        other session each member's rows get a copy."""
        if isinstance(slots, (str, bytes)) or not hasattr(slots, "__len__") or len(slots) < 1:
            raise ValueError("admit_samples: slots must be a list of one or more distinct slots")
        slots = list(slots)
        for r in slots:
            self._check_slot(r)
        if len(set(slots)) != len(slots):
            raise ValueError("admit_samples: slots must be a list of one or more distinct slots")
        self._admit("admit_samples", slots, seed, True, text_hidden, z_style, max_new_tokens, text_mask, ref_hidden,
                    ref_mask, prompt_tokens, start_token, temperature, top_k, top_p, repetition_penalty, logit_bias)

    def _admit(self, who, rows, seed, expand, text_hidden, z_style, max_new_tokens, text_mask, ref_hidden, ref_mask,
               prompt_tokens, start_token, temperature, top_k, top_p, repetition_penalty, logit_bias):
        """One request into the slots `rows` (checked by the caller): what
        admit and admit_samples share.  expand: member j's seed is
        row_seeds(seed, n)[j]; else `seed` itself (one row)."""
        m, eng, g, dev, V = self.m, self.eng, self.g, self.dev, self.V
        n = len(rows)
        # -- checks: nothing is touched before the last of them ----------------
        for name, v in (("temperature", temperature), ("top_k", top_k), ("top_p", top_p), ("seed", seed),
                        ("max_new_tokens", max_new_tokens),
                        ("repetition_penalty", 1.0 if repetition_penalty is None else repetition_penalty)):
            if not _is_scalar(v):
                raise ValueError(f"generate: {name} must be a scalar for one request")
        seeds = ops.row_seeds(int(seed), n) if expand else [seed]
        ctl = DecodeEngine._row_controls(n, [temperature] * n, [top_k] * n, [top_p] * n, seeds, [max_new_tokens] * n,
                                         None if repetition_penalty is None else [repetition_penalty] * n, self.window)
        cap = int(ctl["max_length"][0])
        d = m.token_embed.weight.shape[1]

        def lead(t, dims, name):
            if t is None:
                return None
            if t.dim() == dims - 1:
                t = t[None]
            if t.dim() != dims or t.shape[0] != 1:
                raise ValueError(f"admit: {name} must be one request (unbatched, or a leading 1)")
            return t

        th = lead(text_hidden, 3, "text_hidden")
        z = lead(z_style, 2, "z_style")
        tm, rh, rm = lead(text_mask, 2, "text_mask"), lead(ref_hidden, 3, "ref_hidden"), lead(ref_mask, 2, "ref_mask")
        if not (th.is_cuda and z.is_cuda):
            raise RuntimeError("admit runs on the HIP kernels only (no CPU path)")
        if th.shape[2] != d or (tm is not None and tm.shape[1] != th.shape[1]):
            raise ValueError("admit: text_hidden must be (T_text, d_model) and text_mask (T_text,)")
        S = th.shape[1] + (0 if rh is None else rh.shape[1])
        if S > self.max_keys:
            raise ValueError(f"admit: {S} conditioning keys exceed the session's max_keys = {self.max_keys}")
        if S < 1:
            raise ValueError("admit: the conditioning sequence is empty")
        pt = prompt_tokens[None] if prompt_tokens is not None and prompt_tokens.dim() == 1 else prompt_tokens
        pt, Tp, _ = _check_request(m, 1, cap, pt, start_token, logit_bias, self.pad, self.eos)
        for r in rows:
            if self.state[r] == "lent":
                raise RuntimeError(f"{who}: slot {r} holds the keys of slots {sorted(self.borrowers[r])}, "
                                   "which have not been taken")
            if self.state[r] != "idle":
                raise RuntimeError(f"{who}: slot {r} holds a request that has not been taken")
        # -- conditioning: [ref ‖ text] padded to max_keys, projected once, written into rows[0] and copied from it
        cd, K = self.cd, self.max_keys
        th, tm = m._concat_ref(th.to(cd), tm, rh, rm, 1, dev)
        thp = torch.zeros(1, K, d, device=dev, dtype=cd)
        thp[:, :S] = th
        keep = torch.zeros(1, K, dtype=torch.bool, device=dev)
        keep[:, :S] = True if tm is None else tm.to(dev)
        self.cond.write(rows[0], thp, keep, z)
        for r in rows[1:]:                                  # FP8 keys: quantised once, the other members get the bytes
            self.cond.copy(rows[0], r, keys=not self.share_keys)
        if self.share_keys:
            for r in rows:
                self.cond.point(r, rows[0])
                self.holder[r] = rows[0]
            self.borrowers[rows[0]] = set(rows[1:])
        logits0 = None
        if Tp > 1:                                          # once for the group: states into self.pre
            logits0 = self.pre._prefill(pt.long().to(dev), (thp, z, keep, None, None))       # (1, V)
        for j, r in enumerate(rows):
            for cs, ss in eng.states:
                cs[r].zero_()
                ss[r].zero_()
            # -- slot state and controls
            self.length[r:r + 1].zero_()
            g["draw"][r:r + 1].zero_()
            for name in ("temperature", "top_k", "top_p", "row_seed", "penalty", "max_length"):
                g[name][r:r + 1].copy_(ctl[name][j:j + 1])
            if logit_bias is None:
                g["bias"][r].zero_()
            else:
                g["bias"][r].copy_(logit_bias.to(torch.float32).reshape(V))
            self.finished[r:r + 1].zero_()
            if Tp > 1:
                for (cs, ss), (c1, s1) in zip(eng.states, self.pre.states):
                    cs[r].copy_(c1[0])
                    ss[r].copy_(s1[0])
                eng.set_pos(Tp - 1, slice(r, r + 1))
                self._sample(logits0, slice(r, r + 1))      # token 0 from the prompt's last logits; pos -> Tp
            else:
                eng.tok_buf[r].fill_(int(start_token) if pt is None else 0)
                if pt is not None:
                    eng.tok_buf[r].copy_(pt[0])
                eng.set_pos(0, slice(r, r + 1))
            self.state[r] = "live"

    def _make_idle(self, r):
        eng = self.eng
        self.cond.clear(r)                                  # a borrower reads its own (idle) rows again
        self.holder[r] = r
        self.finished[r:r + 1].fill_(1)
        eng.tok_buf[r].fill_(self.pad)
        eng.set_pos(0, slice(r, r + 1))
        self.state[r] = "idle"

    def poll(self):
        """The slots whose request has finished and has not been taken: one
        copy of finished / length to pinned memory, waited for.  Raises
        IndexError when a step embedded a token id outside token_embed."""
        if self.eng.ctx.fused:
            self.eng._post_token_flag(self.dev)
        self._raw_host.copy_(self._raw, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        self.eng.check_errors()
        n = self.slots
        length = self._raw_host[:8 * n].view(torch.int64)
        fin = self._raw_host[8 * n:].view(torch.int32)
        for s in range(n):
            if self.state[s] == "live" and int(fin[s]) != 0:
                self.state[s] = "done"
                self.lengths[s] = int(length[s])
        return [s for s in range(n) if self.state[s] == "done"]

    @torch.no_grad()
    def take(self, slot, return_logprobs=False):
        """The finished request's tokens, (length,) int64, and the slot idle
        again -- except a slot whose K/V rows other members of its
        admit_samples group still read (a share_keys session): it becomes
        "lent", admit / admit_samples into it raise RuntimeError, and it goes
        idle, its rows zeroed, when the last of them is taken.  return_logprobs, on a session opened with logprobs: (tokens,
        logprobs (length,) fp32), the log-probability recorded beside every
        token (DecodeEngine.generate's return_logprobs has the definition)."""
        self._check_slot(slot)
        if return_logprobs and not self.logprobs:
            raise ValueError("take: return_logprobs needs a session opened with logprobs=True")
        if self.state[slot] == "live":
            self.poll()
        if self.state[slot] != "done":
            raise RuntimeError(f"take: slot {slot} holds no finished request")
        toks = self.g["hist"][slot, :self.lengths[slot]].clone()
        lps = self.g["lp_hist"][slot, :self.lengths[slot]].clone() if return_logprobs else None
        h = self.holder[slot]
        if self.borrowers[slot]:                            # other slots still read this slot's K/V rows: they stay,
            self.state[slot] = "lent"                       # untouched, until the last of those has been taken
        else:
            self._make_idle(slot)
            if h != slot:
                self.borrowers[h].discard(slot)
                if not self.borrowers[h] and self.state[h] == "lent":
                    self._make_idle(h)
        return (toks, lps) if return_logprobs else toks


def _keys(req):
    th, rh = req["text_hidden"], req.get("ref_hidden")
    return th.shape[-2] + (0 if rh is None else rh.shape[-2])


@torch.no_grad()
def generate_requests(model, requests, *, slots, max_keys=None, check_every=16, eos_id=None, pad_id=0,
                      repetition_window=64, return_logprobs=False, share_keys=False, kv_dtype=None):
    """A queue of requests (dicts of DecodeSession.admit's arguments) through
    one session of `slots` rows by the policy of plan_slots.  Returns the
    token tensors in request order, the slot each request ran in and the
    number of replays made; with return_logprobs also, last, the requests'
    log-probability tensors in the same order.  A request may carry
    samples=n: it is n samples of one request (admit_samples with the
    request's seed), admitted in order once n slots are idle -- the requests
    behind it wait with it, so the order stays deterministic -- into the n
    lowest idle slots; its entries in the token list, the slot list and the
    log-probability list are lists of n.  share_keys opens the session with
    it (the samples of a request then read one copy of its keys); no token
    depends on it.  kv_dtype opens the session with it ("fp8": FP8
    conditioning K/V).  With eos_id a row may end before its cap: the
    loop polls, so the slots then differ from plan_slots' (cap-only) answer;
    no token does."""
    requests = list(requests)
    if int(check_every) < 1:
        raise ValueError("generate_requests: check_every must be >= 1")
    if not requests:
        return ([], [], 0, []) if return_logprobs else ([], [], 0)
    want = [r.get("samples") for r in requests]
    for n in want:
        if n is not None and (isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= int(slots)):
            raise ValueError(f"generate_requests: samples must be an integer in [1, slots = {int(slots)}]")
    if max_keys is None:
        max_keys = max(_keys(r) for r in requests)
    ses = model.open_session(slots, max_keys, eos_id=eos_id, pad_id=pad_id, repetition_window=repetition_window,
                             logprobs=bool(return_logprobs), share_keys=share_keys, kv_dtype=kv_dtype)
    lps = [None if n is None else [None] * n for n in want]
    out, where = [None if n is None else [None] * n for n in want], [None] * len(requests)
    left, who = [None] * ses.slots, [None] * ses.slots      # plan_slots' bookkeeping, with (request, member)
    nxt = 0
    while nxt < len(requests) or any(v is not None for v in left):
        while nxt < len(requests):
            free = [s for s in range(ses.slots) if left[s] is None and ses.state[s] == "idle"]
            n = 1 if want[nxt] is None else want[nxt]
            if len(free) < n:
                break
            req = requests[nxt]
            if want[nxt] is None:
                ses.admit(free[0], **req)
                where[nxt] = free[0]
            else:
                ses.admit_samples(free[:n], **{k: v for k, v in req.items() if k != "samples"})
                where[nxt] = free[:n]
            pt = req.get("prompt_tokens")
            for j, s in enumerate(free[:n]):
                left[s] = int(req["max_new_tokens"]) - (1 if pt is not None and pt.shape[-1] > 1 else 0)
                who[s] = (nxt, None if want[nxt] is None else j)
            nxt += 1
        n = min(int(check_every), max(v for v in left if v is not None))
        ses.run(n)
        left = [None if v is None else max(v - n, 0) for v in left]
        done = ses.poll()
        if n == 0 and not done:
            raise RuntimeError("generate_requests: a request passed its cap without finishing")
        for s in done:
            got = ses.take(s, return_logprobs=True) if return_logprobs else (ses.take(s), None)
            i, j = who[s]
            if j is None:
                out[i], lps[i] = got
            else:
                out[i][j], lps[i][j] = got
            left[s] = who[s] = None
    if return_logprobs:
        return out, where, ses.replays, lps
    return out, where, ses.replays
