"""Single-GPU driver of the fused minibatch step (thin wrapper over the C ABI)."""
from . import capi


class SingleGpuTrainer:
    """One shard, one GPU: LRWorker::update / FMWorker::update on device-resident batches."""

    def __init__(self, model="lr", optimizer="ftrl", k=10, capacity=1 << 22, seed=7,
                 rank=0, world=1, fm_mode="reference", feature_values=False, fields=None,
                 **hyper):
        """fm_mode (FM): "reference" (the reference's pooled second-order term), "canonical"
        (Rendle's per-factor form) or "field_aware" (k factors per field: fields=F, v rows F k
        wide, compile(..., fgid=...)); the last two start the v table hash-normal for both
        optimizers.  feature_values: a nonzero contributes x = val instead of 1
        (compile(..., values=...)); LR, or FM with fm_mode="canonical" / "field_aware"."""
        assert world == 1
        assert fm_mode in capi.FM_MODES, fm_mode
        assert not feature_values or model == "lr" or fm_mode != "reference", \
            "feature_values with FM needs fm_mode='canonical' or 'field_aware'"
        assert fm_mode != "field_aware" or (model == "fm" and fields), \
            "fm_mode='field_aware' needs model='fm' and fields=F"
        self.fields = int(fields) if fm_mode == "field_aware" else 0
        self.feature_values = bool(feature_values)
        opt = capi.OPT_FTRL if optimizer == "ftrl" else capi.OPT_SGD
        self.model = model
        self.fm_mode = fm_mode if model == "fm" else "reference"
        self.w = capi.Table(opt, 1, capi.INIT_ZERO, capacity=capacity, **hyper)
        self.v = None
        if model == "fm":
            hashnorm = opt == capi.OPT_FTRL or self.fm_mode != "reference"
            init = capi.INIT_HASHNORM if hashnorm else capi.INIT_CONST
            vdim = k * self.fields if self.fields else k
            self.v = capi.Table(opt, vdim, init, 0.001, seed=seed, capacity=capacity, **hyper)
        self.ws = capi.Workspace()
        if self.fields:
            self.ws.fm_fields(self.fields)
        if self.fm_mode != "reference":
            self.ws.fm_mode(self.fm_mode)

    def compile(self, rowptr, keys, labels, values=None, fgid=None):
        assert (values is not None) == self.feature_values, \
            "values go with SingleGpuTrainer(feature_values=True)"
        if self.fields:          # a fielded minibatch always takes the generic build
            assert fgid is not None, "fm_mode='field_aware': compile(..., fgid=...)"
            return capi.Batch(rowptr, keys, labels, on_gpu=True, values=values,
                              fields=self.fields, fgid=fgid)
        if self.feature_values:
            assert values is not None, "feature_values=True: compile(..., values=...)"
            # LR: straight to state rows and cells that carry the values, as the one-rank
            # trainer's compile (capi.tune("valued_lr", 1) pins the generic build); FM: the
            # generic build
            if self.model == "lr" and capi.tuned("valued_lr") != 1:
                return capi.LocalBatch(self.w, rowptr, keys, labels, values=values)
            return capi.Batch(rowptr, keys, labels, on_gpu=True, values=values)
        assert values is None, "values need SingleGpuTrainer(feature_values=True)"
        if self.model == "lr":   # sort-free key build against the table (cells)
            return capi.LocalBatch(self.w, rowptr, keys, labels)
        return capi.Batch(rowptr, keys, labels).upload()

    def step(self, batch, stream=None):
        if self.model == "lr":
            capi.lr_step(self.w, batch, self.ws, stream)
        else:
            capi.fm_step(self.w, self.v, batch, self.ws, stream)

    def predict(self, batch):
        if self.model == "lr":
            return capi.lr_predict(self.w, batch, self.ws)
        return capi.fm_predict(self.w, self.v, batch, self.ws)

    def defrag(self):
        """renumber state rows in key order (call when the key set has settled)"""
        self.w.defrag()
        if self.v is not None:
            self.v.defrag()

    def check(self):
        self.w.check()
        if self.v is not None:
            self.v.check()

    def profile(self, enable):
        self.ws.profile(enable)

    def profile_read(self):
        return self.ws.profile_read()
