"""my_environment.utils: the behaviour-cloning kick-start (``imitation_kickstarter``)."""
