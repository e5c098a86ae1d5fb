"""Drop-ins for the reference's ``utils/`` scripts that have a device path here."""
