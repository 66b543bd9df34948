"""The launches of a training step that wait to leave inside other launches, and who may send them off when."""
import contextlib

import torch


class StepQueue:
    """One instance per process (ops.STEP).  A captured step saves kernel nodes by letting small launches ride in others:

    Slab sums.  Several backward nodes end in "out = sum over R partial slabs" kernels whose results only the optimizer reads
    (weight gradients of the row-split GEMMs), each a ~5 us node of the captured step whatever its size.  A node may hand
    (slabs, out) to defer_slab_sum instead of launching, and ONE launch at the end of the backward pass (autograd's
    queue_callback -> finish) sums them all: the gradients are complete when backward() returns, as before.  Deferring hands
    autograd a gradient tensor that is not written yet, which is only safe when AccumulateGrad takes the buffer over as it is:
    the target parameter has no gradient yet (otherwise `p.grad += out` would read the unwritten buffer: a second backward
    before a step, zero_grad(set_to_none=False)) and no hook that reads it.  So the permission is scoped twice: a model grants
    it for the duration of ITS training forward (`with deferring(on)`: every parameter of it feeds exactly one backward node
    per layer / order), the forward of a node snapshots it (ctx.defer = ops.defer_scope()), and the backward asks
    ops.can_defer(ctx.defer, params) when it gets there - anything else launches the sum on the spot.  A backward pass that
    raised leaves its sums behind (the engine drops its callbacks); the next outermost deferring() forgets them: their buffers
    belong to a graph that is gone, and a non-empty list would keep the next pass from registering its own callback.

    Waiting tn products.  The weight gradients of an MSHGNN layer (hgat._weight_grads) and those of the k-gram GRU
    (gru.GRUExpandAll._weight_grads) are the same kernel over two problem lists, and only the optimizer (and the slab sums) read
    either.  The layer may hand its list to defer_product instead of launching - under the permission above, asked for ALL the
    weights it writes, since autograd is handed their buffers unwritten - and the GRU node, which runs later in the backward
    pass, calls leave_with(its own list): the waiting lists that fit beside it in one problem table leave in the SAME launch
    (two families, ops._launch_tn_products), the others on their own directly in front.  One invariant keeps the gradients
    right: a waiting product is issued before any slab sum (its slabs may be among the sum's inputs) and before anyone outside
    the backward pass can read what it writes - flush(), finish() and an immediate sum all issue the waiting products first,
    and finish() is also where they leave when no GRU node follows the layer (order 1).  The keepalive of a waiting product
    (its operands, which autograd would free with the node) is dropped only after its launch has been issued.

    Step-scalar rider.  Before the backward pass of a captured step optim.FusedAdam.hyper_rider offers the arguments of its
    srec_adam_hyper_multi launch (offer_rider); the end-of-backward launch takes them along when sums are waiting and
    FusedAdam.launch asks rider_result() which slots were advanced - None: nobody took the rider, launch() runs its own
    kernel.  The kernel advances the (0, 0) step counter the dropout masks are keyed by, and a backward node that runs after a
    mid-backward flush (dist.VocabParallel.bucket_ready) re-derives its forward's masks from that counter.  Hence two ways to
    send the sums off: flush() from INSIDE a backward pass, which cannot touch the rider, and finish() once the pass is
    complete (the engine's callback, FusedAdam._work), the only taker of the rider.

    Batch intake.  graph.GraphedTrainStep offers the mailbox intake entries of the step it captures, (mailbox, M, counter, dst,
    cap, err, ...) as srec_copy_words_mailbox takes them (offer_intake).  A model with a prologue launch lets one ride in it
    (ops.step_prologue -> take_intake; the others leave ahead of it); any other model launches them ahead of its first read
    of the batch (flush_intake in the lookup).  The capture checks intake_pending() after the forward.

    abort() forgets everything that waits: a capture that died, or a captured step the ranks agreed to drop.

    The launches themselves are the callables given here (ops._launch_slab_sums(tasks, rider), ops._launch_intake(*entry[:6]),
    ops._launch_tn_products(family_a, family_b): either family may be None)."""

    def __init__(self, launch_slab_sums, launch_intake, launch_products=None):
        self._launch_slab_sums, self._launch_intake, self._launch_products = launch_slab_sums, launch_intake, launch_products
        self._on, self._depth = False, 0
        self._sums, self._intake = [], []
        self._products = []                            # [(problems, keepalive)] in waiting order
        self._rider, self._done = None, None           # (args, slots, keepalive) on offer; the slots a finish() advanced

    # ---- deferral permission
    @property
    def may_defer(self):
        return self._on

    @contextlib.contextmanager
    def deferring(self, on):
        prev = self._on
        if not self._depth:
            self.drop_stale()
        self._depth += 1
        self._on = bool(on)
        try:
            yield
        finally:
            self._depth -= 1
            self._on = prev

    def _in_backward(self):
        """may something start to wait?  Registers finish() with the running backward pass unless something already waits"""
        if self._sums or self._products:
            return True
        try:
            torch.autograd.Variable._execution_engine.queue_callback(self.finish)
        except RuntimeError:                            # not inside a backward pass: nothing to wait for
            return False
        return True

    # ---- slab sums
    def defer_slab_sum(self, part, out, ok=True, tall=False):
        """out [n] (any shape, contiguous) = sum over the leading dimension of part [R, n...]: now, or (ok) deferred to the
        end of the running backward pass.  tall: few columns, hundreds of rows (bias partials)"""
        if not (ok and self._in_backward()):
            self._issue_products()                      # (part may be the slabs of a waiting product)
            self._launch_slab_sums([(part, out, tall)])
            return
        # (an ALIAS of out: autograd takes a returned gradient as it is only when nothing else refers to the tensor object -
        #  with a second reference AccumulateGrad would clone it, before the sum has been written)
        self._sums.append((part, out.detach(), tall))

    def waiting(self):
        return len(self._sums)

    def drop_stale(self):
        self._sums, self._products = [], []

    # ---- tn products
    def defer_product(self, probs, keepalive=None, ok=True):
        """probs: the problem list of one tn launch (at most one problem table).  Now, or (ok) waiting for leave_with / the next
        flush() / finish() of the running backward pass; keepalive: what the problems read, held until the launch is issued"""
        if ok and self._in_backward():
            self._products.append((list(probs), keepalive))
        else:
            self._launch_products(list(probs), None)

    def products_waiting(self):
        return len(self._products)

    def leave_with(self, probs, maxp):
        """the caller's own tn launch over probs (<= maxp problems, maxp = one problem table): waiting lists ride along as the
        other family as long as they fit whole, in waiting order; the rest leave on their own directly in front"""
        waiting, self._products = self._products, []
        room, taken, rest = maxp - len(probs), [], []
        for e in waiting:
            if len(e[0]) <= room:
                taken.append(e)
                room -= len(e[0])
            else:
                rest.append(e)
        for e in rest:
            self._launch_products(e[0], None)
        self._launch_products([q for e in taken for q in e[0]] or None, list(probs))

    def _issue_products(self):
        waiting, self._products = self._products, []
        for e in waiting:
            self._launch_products(e[0], None)

    def flush(self):
        """from inside the backward pass: launch the waiting products, then the waiting sums; the rider stays"""
        self._issue_products()
        if self._sums:
            tasks, self._sums = self._sums, []
            self._launch_slab_sums(tasks, None)

    def finish(self):
        """the backward pass is complete: launch the waiting products, then the waiting sums, and the rider with them"""
        self._issue_products()
        if self._sums:
            tasks, self._sums = self._sums, []
            rider, self._rider = self._rider, None
            self._launch_slab_sums(tasks, rider[0] if rider is not None else None)
            if rider is not None:
                self._done = rider[1]

    # ---- step-scalar rider
    def offer_rider(self, args, slots, keepalive=None):
        """args: those of srec_adam_hyper_multi without the stream; keepalive: what they point into, held until the launch"""
        self._rider, self._done = (args, frozenset(slots), keepalive), None

    def rider_result(self):
        """frozenset of the slots a finish() advanced, or None; the rider is withdrawn either way"""
        done, self._rider, self._done = self._done, None, None
        return done

    # ---- batch intake
    def offer_intake(self, entries):
        self._intake = list(entries)

    def intake_pending(self):
        return bool(self._intake)

    def flush_intake(self):
        while self._intake:
            self._launch_intake(*self._intake.pop(0)[:6])

    def take_intake(self):
        """-> the entry the caller's own launch carries (or None); the others leave ahead of it"""
        box = self._intake.pop() if self._intake else None
        self.flush_intake()
        return box

    def abort(self):
        self._sums, self._products, self._intake, self._rider, self._done = [], [], [], None, None
