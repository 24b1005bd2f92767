"""Process-wide tuning knobs pinned for a block of a GPU test - test infrastructure."""


class pinned:
    """The knobs (option name -> (value, default)) set on entry and back at their defaults on exit, where the options named in
    `restore` - launch-mode switches the block may have turned - go back to 1, their default."""

    def __init__(self, eng, knobs, restore=("fused_stack",)):
        self.eng, self.knobs, self.restore = eng, knobs, restore

    def __enter__(self):
        for k, (v, _) in self.knobs.items():
            self.eng.set_option(k, v)

    def __exit__(self, *exc):
        for k, (_, v) in self.knobs.items():
            self.eng.set_option(k, v)
        for k in self.restore:
            self.eng.set_option(k, 1)
