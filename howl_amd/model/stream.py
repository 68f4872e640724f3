"""What the one-launch streaming sessions share (``Res8StreamSession`` of ``cnn.py``; ``LstmStreamSession``, ``GruStreamSession`` and
``LasStreamSession`` of ``rnn.py``); a session supplies the texts of its two refusals, its range query, its hooks and its launch."""
import torch

from howl_amd import ops

__all__ = ["PreparedStreamSession", "StreamSession"]


class StreamSession:
    """One model behind ``std`` (``StandardAudioTransform``) and ``zmuv`` (``ZmuvTransform`` or None): ``probabilities(pcm, ...)`` takes
    raw PCM to class probabilities in ONE kernel launch.  Eval mode only, standard filterbank only; a session owns whatever it
    allocates, so two engines on two streams share nothing.

    A subclass sets ``RUNS`` (what the kernel runs that training mode would not: the text of the training-mode refusal), ``UNIT``
    (what a row of ``pcm`` is called in the shape refusal) and ``in_range`` (its ``ops.*_stream_supported``)."""
    RUNS = None
    UNIT = "windows"
    in_range = None

    def __init__(self, model, std, zmuv):
        self.model, self.std, self.zmuv = model, std, zmuv
        self._ws = None
        self._frames = {}
        self._asked = (None, False)      # the last (n_samples, n_mels, n_labels) the library was asked about, and its answer

    def supported(self, n_samples: int) -> bool:
        """Rows of ``n_samples`` samples are inside the kernel's range (the class's docstring has it) and the frontend would not
        draw a VTLP filterbank for them."""
        if self.std.augment_params[0].enabled and self.std.training:
            return False
        # the range depends on these three numbers alone, and a stream asks for the same three twice per window (the engine, then
        # probabilities()): the library is asked when they change
        key, asked = (n_samples, self.std.n_mels, self.model.num_labels), self._asked
        if key != asked[0]:
            asked = self._asked = (key, self.in_range(*key))
        return asked[1]

    def _enter(self, pcm):
        """The head of every ``probabilities()``, in this order: the training-mode refusal, the shape refusal, then the frontend's
        draw -- a refused call leaves ``std.rand`` where it was."""
        if self.model.training:
            raise RuntimeError(f"{type(self).__name__} runs {self.RUNS}: call model.eval() first")
        if pcm.dim() != 2 or not self.supported(pcm.size(1)):
            raise ValueError(f"{type(self).__name__}: {self.UNIT} of shape {tuple(pcm.shape)} are outside the streaming kernel's range "
                             f"(see supported()); use the model's forward")
        if self.std.augment_params[0].enabled:
            self.std.rand.random()      # the frontend's draw happens on every call, eval mode included: keep the stream's position

    def _pair(self):
        return self.zmuv.pair() if self.zmuv is not None else None

    def _frames_of(self, L: int) -> int:
        """``std.compute_lengths`` of an ``L``-sample window (it depends on the window's size alone: computed once per size)."""
        if L not in self._frames:
            self._frames[L] = int(self.std.compute_lengths(torch.tensor([L]))[0])
        return self._frames[L]

    def _workspace(self, need: int, device):
        """The session's scratch, at least ``need`` bytes on ``device``: grown on demand, never shrunk."""
        if self._ws is None or self._ws.device != device or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws


class PreparedStreamSession(StreamSession):
    """A session whose kernel reads a prepared state (packed weights, folded BatchNorms) instead of the model's tensors.  The state
    is prepared again whenever one of the ``_watched()`` tensors was replaced or written through torch since the last launch
    (``data_ptr()`` / ``_version``: ``load_state_dict``, an optimiser step); writes that torch does not see need ``refresh()``.
    A subclass supplies ``_watched()``, ``_state_bytes()`` and ``_prepare(state)``."""

    def __init__(self, model, std, zmuv):
        super().__init__(model, std, zmuv)
        self._state = None
        self._key = None

    def refresh(self):
        """Forces the next call to prepare the state again."""
        self._key = None

    def _watched(self):
        """The tensors the prepared state is made from; ``_state_bytes()`` is its size and ``_prepare(state)`` makes it (uint8)."""
        raise NotImplementedError

    def _prepared_state(self, device):
        key = tuple((t.data_ptr(), t._version) for t in self._watched())
        if self._state is None or self._state.device != device or key != self._key:
            if self._state is None or self._state.device != device:
                self._state = torch.empty(self._state_bytes(), dtype=torch.uint8, device=device)
            self._prepare(self._state)
            self._key = key
        return self._state
